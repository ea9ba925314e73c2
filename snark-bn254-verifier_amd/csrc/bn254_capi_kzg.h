// bn254_capi_kzg.h -- what bn254_capi_kzg.hip offers the probe of bn254_capi_dbg.hip (bn254_dbg_kzg_fold).  Private like bn254_capi_internal.h.
#pragma once
#include "bn254_capi_internal.h"

#define KZG_RLC_MIN_FLOOR 64
// BN254_FLAG_RLC is honoured from this many openings per launch on unless bn254_set_kzg_params / BN254_KZG_RLC_MIN say otherwise: the smallest measured size at
// which the weighted call beats the exact one by more than the spread (profiles/r17_kzg_batch.txt: a tie at 4096, 0.48 of the exact time at 65 536, 0.38 at 262 144)
#define KZG_RLC_MIN_DEFAULT 65536

// where a launch leaves the probe's values (device memory): per opening F and H' (64 bytes each) and two identity flags; per group the same and the group's status
// fold (batch-opening records only): per record the digest gamma is reduced from and y^, 32 bytes each
struct KzgProbeDev { uint8_t *f, *h, *inf, *grp_f, *grp_h, *grp_inf, *grp_st, *fold = nullptr; };
// the caller's buffers: n x 64, n x 64, n x 2, groups x 131 (F | H' | two flags | status) or null, n x 64 (batch-opening records) or null
struct KzgProbeHost { uint8_t *f, *h, *inf, *grp, *fold = nullptr; };
// what the records of a call are: openings (k = 0), or batch-opening proofs of k digests and data_len bytes of caller data each (bn254_kzg_verify_folded_batch)
struct KzgForm {
  int k = 0, data_len = 0;
  size_t rec_len() const;
  int n_terms(bool weighted) const;
  int n_var(bool weighted) const;      // variable terms of both sums
  size_t max_launch() const;
};

#pragma GCC visibility push(hidden)
int kzg_check_args(const void* key, const void* openings, size_t stride, size_t n, const void* status, unsigned flags, bool host_key, bool* done, const KzgForm& form = KzgForm());
// the limits of a batch-opening call: 1 <= n_digests <= BN254_KZG_FOLD_MAX_DIGESTS, data_len <= BN254_KZG_FOLD_MAX_DATA
int kzg_fold_form(size_t n_digests, size_t data_len, KzgForm* form);
// weights: null, or n x 16 bytes (big-endian, forced odd) in the ChaCha20 stream's place; force_weighted: the weighted form whatever the knob says (the probe)
int kzg_host_call(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, uint8_t* status, int device, unsigned flags, int force, const uint8_t* weights, bool force_weighted,
                  KzgProbeHost* ph, const KzgForm& form = KzgForm());
int kzg_fold_on_host(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, const uint8_t* weights, unsigned flags, bool weighted, KzgProbeHost& ph, uint8_t* status,
                     const KzgForm& form = KzgForm());
#pragma GCC visibility pop
