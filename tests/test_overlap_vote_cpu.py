"""The stream-overlap decision of a Groth16 (key, device) -- csrc/bn254_overlap_vote.h, the functions g16_enqueue_exact calls -- replayed without a device through
bn254_dbg_overlap_replay.  The rule is the one include/bn254_verify.h states for bn254_groth16_stream_overlap: a batch's measurement is read by the NEXT batch; three
readings in a row below 1.15 ("one after the other") switch the device to one sub-batch per launch, one reading at or above it settles the question the other way; on
one sub-batch per launch every 256th batch runs two again and is measured, and that one reading decides; BN254_STREAM_FALLBACK=0 reports only.  Every expected row
below is written out from that rule and the three constants (3, 256, 1.15), batch by batch: (probe_now, single_stream the batch is planned with, state after the
batch -- 0 open, 1 this batch is being measured, 2 settled --, serial readings in a row, last ratio read)."""
import struct

SERIAL = (1.0, 1.0, 1.0, 2.0)      # part 1 runs from 1 to 2 ms after part 0 began, both take 1 ms: 2 ms of work in a union of 2 ms, ratio 1.0
SIDE = (1.0, 1.0, 0.0, 1.0)        # both from 0 to 1 ms: 2 ms of work in a union of 1 ms, ratio 2.0


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def test_three_serial_readings_switch_and_the_fourth_batch_is_the_first_on_one_stream(pkg):
    got = pkg.dbg_overlap_replay([SERIAL] * 6)
    assert got == [(0, 0, 1, 0, -1.0),     # nothing to read yet; measured
                   (0, 0, 1, 1, 1.0),      # reads batch 1: one vote; measured
                   (0, 0, 1, 2, 1.0),      # reads batch 2: two votes; measured
                   (0, 1, 2, 3, 1.0),      # reads batch 3: the third vote -- this batch is the first planned with single_stream; one sub-batch is not measured
                   (0, 1, 2, 3, 1.0),
                   (0, 1, 2, 3, 1.0)]


def test_two_serial_readings_do_not_switch(pkg):
    got = pkg.dbg_overlap_replay([SERIAL, SERIAL, None, None, None])
    assert got == [(0, 0, 1, 0, -1.0),
                   (0, 0, 1, 1, 1.0),
                   (0, 0, 0, 2, 1.0),      # reads batch 2: two votes, the question stays open; a batch that cannot be measured
                   (0, 0, 0, 2, 1.0),
                   (0, 0, 0, 2, 1.0)]


def test_a_side_by_side_reading_settles_it(pkg):
    got = pkg.dbg_overlap_replay([SERIAL, SERIAL, SIDE, SERIAL, SERIAL, SERIAL, SERIAL])
    assert got == [(0, 0, 1, 0, -1.0),
                   (0, 0, 1, 1, 1.0),
                   (0, 0, 1, 2, 1.0),
                   (0, 0, 2, 0, 2.0)] + [(0, 0, 2, 0, 2.0)] * 3      # reads batch 3: votes back to 0, settled; never measured again while on two streams


def test_the_threshold_is_1_15(pkg):
    """1.1499 reads "one after the other", 1.15 does not.  Two parts of a ms each that end 2 ms after part 0 began: ratio 2a / 2, exact in binary floating point."""
    below = (1.1499, 1.1499, 2.0 - 1.1499, 2.0)
    at = (1.15, 1.15, 2.0 - 1.15, 2.0)
    got = pkg.dbg_overlap_replay([below] * 4)
    assert got[3] == (0, 1, 2, 3, f32(1.1499)) and [g[3] for g in got] == [0, 1, 2, 3]
    got = pkg.dbg_overlap_replay([at] * 4)
    assert got == [(0, 0, 1, 0, -1.0)] + [(0, 0, 2, 0, f32(1.15))] * 3      # the first reading settles it: side by side
    # a reading at the threshold between two below it: the count starts over, and the question is settled
    got = pkg.dbg_overlap_replay([below, at, below, below])
    assert got == [(0, 0, 1, 0, -1.0), (0, 0, 1, 1, f32(1.1499)), (0, 0, 2, 0, f32(1.15)), (0, 0, 2, 0, f32(1.15))]


def _pinned_then(probe_timings, more):
    """Batches 1 .. 3 are measured serial, batch 4 is the first on one stream, so the 256th batch on one stream is batch 259: it gets probe_timings."""
    return [SERIAL] * 258 + [probe_timings] + [SERIAL] * more


def test_on_one_stream_every_256th_batch_probes_and_a_serial_reading_repins_at_once(pkg):
    got = pkg.dbg_overlap_replay(_pinned_then(SERIAL, 257))
    assert got[3:258] == [(0, 1, 2, 3, 1.0)] * 255       # batches 4 .. 258, the 1st .. 255th on one stream: no probe, not measured
    assert got[258] == (1, 0, 1, 3, 1.0)                 # batch 259, the 256th: planned with two streams and measured
    assert got[259] == (0, 1, 2, 4, 1.0)                 # batch 260 reads it: ONE serial reading and the device is on one stream again
    assert got[260:514] == [(0, 1, 2, 4, 1.0)] * 254     # batches 261 .. 514, the 258th .. 511th
    assert got[514] == (1, 0, 1, 4, 1.0)                 # batch 515, the 512th: the next probe
    assert got[515] == (0, 1, 2, 5, 1.0)


def test_a_side_by_side_reading_on_a_probe_restores_two_streams(pkg):
    got = pkg.dbg_overlap_replay(_pinned_then(SIDE, 300))
    assert got[258] == (1, 0, 1, 3, 1.0)
    assert got[259:] == [(0, 0, 2, 0, 2.0)] * 300        # back to two sub-batches side by side, settled: no probe at what would have been the 512th batch


def test_fallback_off_reports_only(pkg):
    got = pkg.dbg_overlap_replay([SERIAL] * 300, fallback=False)
    assert got[:3] == [(0, 0, 1, 0, -1.0), (0, 0, 1, 1, 1.0), (0, 0, 1, 2, 1.0)]
    assert got[3:] == [(0, 0, 2, 3, 1.0)] * 297          # three votes, settled, single_stream stays 0: nothing to probe either


def test_timing_unavailable_settles_and_changes_nothing_else(pkg):
    assert pkg.dbg_overlap_replay(["untimed", SERIAL, SERIAL]) == [(0, 0, 1, 0, -1.0), (0, 0, 2, 0, -1.0), (0, 0, 2, 0, -1.0)]
    got = pkg.dbg_overlap_replay([SERIAL, SERIAL, "untimed", SERIAL, SERIAL])
    assert got == [(0, 0, 1, 0, -1.0), (0, 0, 1, 1, 1.0), (0, 0, 1, 2, 1.0), (0, 0, 2, 2, 1.0), (0, 0, 2, 2, 1.0)]      # votes and ratio as they were


def test_ratio(pkg):
    """Sum of the two durations / their union, the union from the earlier start to the later end, at least 1e-6 ms."""
    def ratio(t):
        return pkg.dbg_overlap_replay([t, None])[1][4]
    assert ratio(SERIAL) == 1.0 and ratio(SIDE) == 2.0
    assert ratio((2.0, 2.0, 1.0, 3.0)) == f32(4.0 / 3.0)           # half overlapped: 4 ms of work from 0 to 3
    assert ratio((2.0, 2.0, -1.0, 1.0)) == f32(4.0 / 3.0)          # the second part started first (s1 < 0): from -1 to 2
    assert ratio((1.0, 3.0, -4.0, -1.0)) == f32(4.0 / 5.0)         # ... and ended before part 0 began: from -4 to 1
    assert ratio((3.0, 1.0, 1.0, 2.0)) == f32(4.0 / 3.0)           # part 1 inside part 0: the union is part 0
    assert ratio((0.0, 0.0, 0.0, 0.0)) == 0.0                      # a union of no length: the floor, not a division by zero
    assert ratio((2.0 ** -21, 2.0 ** -21, 0.0, 2.0 ** -21)) == f32(f32(2.0 ** -20) / f32(1e-6))      # 0.48 us side by side: under the floor of 1e-6 ms
