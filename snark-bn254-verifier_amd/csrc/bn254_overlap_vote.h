// bn254_overlap_vote.h -- do the sub-batch streams of a Groth16 batch run side by side?  The decision as a value and PURE functions of it (no HIP, nothing of the
// library): g16_enqueue_exact (bn254_capi_g16.hip) queries and records the four events and writes the diagnostic, everything it decides from them is here, and
// bn254_dbg_overlap_replay runs the same functions on given timings (tests/test_overlap_vote_cpu.py).  One measurement decides nothing (another tenant's kernels, a
// profiler that serialises dispatches): OV_AGREE in a row must read "one after the other" before the plan changes, one that reads "side by side" settles it the other
// way; once on one sub-batch per launch, every OV_REPROBE-th batch runs two again and is measured, so that a transient cause does not pin the key to the slower plan.
#pragma once
#include <stddef.h>
#include <string>

namespace bn254 {

#define OV_AGREE 3
#define OV_REPROBE 256
#define OV_SERIAL_BELOW 1.15f   // sum of the two durations / their union: about 2 side by side, about 1 one after the other

struct OvVote {
  int state = 0;                // 0: open -- the next two-stream batch is measured; 1: events recorded, not read yet; 2: settled
  float ratio = -1.f;           // the last measurement read; -1: none yet
  bool single_stream = false;   // one sub-batch per launch (the `single_stream` of g16_plan_chunk, except on a probe)
  int serial_votes = 0;         // measurements in a row that read "one after the other"
  unsigned batches = 0;         // batches begun on one sub-batch per launch
  bool probe = false;           // the measurement under way is a re-probe
  std::string diag;             // the explanation, per (key, device): bn254_groth16_stream_overlap hands it to bn254_last_diagnostic() of the calling thread
};

// part 0 ran for a0 ms, part 1 for a1 ms from s1 to e1 ms after part 0 began (s1 < 0: it began first)
inline float ov_ratio(float a0, float a1, float s1, float e1) {
  const float lo = s1 < 0 ? s1 : 0, hi = e1 > a0 ? e1 : a0;
  return (a0 + a1) / (hi - lo > 1e-6f ? hi - lo : 1e-6f);
}

// The recorded measurement (state 1) is read.  ratio: null when the event timings could not be had, which settles the question as it stands.  fallback:
// BN254_STREAM_FALLBACK, false reports only.  OV_SERIALISED / OV_RESTORED: the caller writes the diagnostic
enum OvChange { OV_UNCHANGED = 0, OV_SERIALISED = 1, OV_RESTORED = 2 };
inline OvChange ov_read(OvVote& v, const float* ratio, bool fallback) {
  OvChange change = OV_UNCHANGED;
  if (ratio) {
    v.ratio = *ratio;
    if (v.ratio < OV_SERIAL_BELOW) {
      v.serial_votes++;
      if (v.serial_votes >= OV_AGREE || v.probe) { v.single_stream = fallback; change = OV_SERIALISED; }
    } else {
      v.serial_votes = 0;
      if (v.single_stream) change = OV_RESTORED;
      v.single_stream = false;
    }
    // keep measuring until the question is settled either way: OV_AGREE agreeing answers
    v.state = (v.serial_votes > 0 && v.serial_votes < OV_AGREE && !v.single_stream) ? 0 : 2;
  } else v.state = 2;
  v.probe = false;
  return change;
}

// A batch begins (after ov_read, if there was something to read).  true: this batch is a re-probe -- it is planned with two streams and measured
inline bool ov_begin_batch(OvVote& v) {
  if (!(v.single_stream && v.state == 2 && ++v.batches % OV_REPROBE == 0)) return false;
  v.probe = true; v.state = 0;
  return true;
}

// Is this chunk measured?  The first two sub-batches of a chunk that runs several side by side, while the question is open -- and only when the two are of
// (nearly) equal size: a short second part beside a long first one reads as "no overlap" whatever the queues do
inline bool ov_measures(const OvVote& v, bool concurrent, int parts, size_t count0, size_t count1) {
  return concurrent && parts >= 2 && v.state == 0 && count1 * 10 >= count0 * 9;
}

}  // namespace bn254
