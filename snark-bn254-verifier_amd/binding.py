"""ctypes binding of libbn254_verify_amd.so.  Mirrors the reference's API names (verifier/src/lib.rs:29-49):
Groth16Verifier.verify(proof, vk, public_inputs) plus the new verify_batch."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REJECT, ACCEPT, ERR_NOT_MEMBER, ERR_NOT_ON_CURVE, ERR_NOT_IN_SUBGROUP, ERR_INPUT_LEN, ERR_MALFORMED = range(7)
VK_REFERENCE, VK_GNARK = 0, 1
FLAG_STRICT_SCALARS, FLAG_RLC, FLAG_COMPRESSED_PROOFS = 1, 2, 4
COMPRESSED_PROOF_LEN = 128   # gnark's compressed Groth16 proof: A (32) | B (64) | C (32)
RAW_PROOF_LEN = 324
NUM_KERNELS = 4
ABI_VERSION = 5   # include/bn254_verify.h: BN254_ABI_VERSION


E_SELFTEST = -6      # BN254_E_SELFTEST: the device failed its known-answer self-test and is refused
SELFTEST_NUM_CHECKS = 10


class Bn254Error(RuntimeError):
    """An infrastructure error of the C ABI; `code` is the BN254_E_* value (None where the binding itself refuses)."""
    code = None


class Bn254SelfTestError(Bn254Error):
    """BN254_E_SELFTEST: a shipped kernel disagrees with its known answer on the device (device_selftest); the text names the check."""
    code = E_SELFTEST


def lib_path():
    # BN254_LIB_PATH: a diagnostics build of the same library (tools/plonk_stage_marks.py); never set in tests or the bench
    return os.environ.get("BN254_LIB_PATH") or os.path.join(HERE, "libbn254_verify_amd.so")


def build(verbose=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc"), "-j2"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return lib_path()


_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process, whatever the import order.  The library needs `libamdhip64.so.7` (soname); a PyTorch-ROCm wheel bundles
    its own copy of that runtime and asks for it as `libamdhip64.so` (no version), so the dynamic loader only recognises the two requests as
    the same object when torch's copy is mapped FIRST.  Mapped the other way round the process ends up with two runtimes and the second one
    sees no devices (the library then answers BN254_E_NO_DEVICE).  So when a torch with a bundled runtime is installed and not yet imported,
    its copy is mapped here, before the library -- without importing torch.  A host without torch (the C++ / Rust case) is not affected."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    rt = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(lib_path()):
            raise Bn254Error("libbn254_verify_amd.so is not built (run __graft_entry__.build()); there is no fallback path")
        _share_torch_hip_runtime()
        L = C.CDLL(lib_path())
        L.bn254_last_error.restype = C.c_char_p
        L.bn254_version.restype = C.c_char_p
        L.bn254_status_string.restype = C.c_char_p
        L.bn254_groth16_kernel_name.restype = C.c_char_p
        L.bn254_groth16_vk_num_public.restype = C.c_size_t
        L.bn254_synth_groth16_vk_len.restype = C.c_size_t
        L.bn254_groth16_vk_prepare.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p)]
        L.bn254_groth16_vk_free.argtypes = [C.c_void_p]
        L.bn254_groth16_vk_num_public.argtypes = [C.c_void_p]
        L.bn254_groth16_verify_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
        L.bn254_groth16_verify_batch_multi.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint]
        L.bn254_groth16_proof_write_raw.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p]
        L.bn254_groth16_verify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        L.bn254_groth16_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        L.bn254_plonk_last_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_size_t)]
        L.bn254_groth16_rlc_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint)]
        L.bn254_groth16_verify.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_uint, C.c_void_p]
        L.bn254_groth16_last_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.bn254_synth_groth16.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bn254_synth_groth16_vk_len.argtypes = [C.c_size_t]
        L.bn254_synth_groth16_range.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bn254_shard_plan.argtypes = [C.c_size_t, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.bn254_plonk_vk_prepare.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.bn254_plonk_vk_free.argtypes = [C.c_void_p]
        L.bn254_plonk_vk_num_public.argtypes = [C.c_void_p]
        L.bn254_plonk_vk_num_public.restype = C.c_size_t
        L.bn254_plonk_verify_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]
        L.bn254_plonk_verify_batch_flags.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
        L.bn254_plonk_verify.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p]
        L.bn254_plonk_verify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        L.bn254_plonk_verify_batch_multi.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint]
        L.bn254_plonk_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        L.bn254_plonk_footprint.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        if L.bn254_abi_version() != ABI_VERSION:
            raise Bn254Error("libbn254_verify_amd.so has ABI revision %d, this binding was written for %d" % (L.bn254_abi_version(), ABI_VERSION))
        L.bn254_groth16_kernel_kind_name.restype = C.c_char_p
        L.bn254_groth16_kernel_kind_name.argtypes = [C.c_int]
        L.bn254_set_profile_kernels.argtypes = [C.c_uint]
        L.bn254_set_rlc_params.argtypes = [C.c_long, C.c_int, C.c_long]
        L.bn254_set_rlc_params.restype = None
        L.bn254_groth16_kernel_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_size_t)]
        L.bn254_groth16_kernel_profile_all.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def kernel_kinds():
    return [lib().bn254_groth16_kernel_kind_name(i).decode() for i in range(lib().bn254_groth16_num_kernel_kinds())]


def set_profile_kernels(names=None):
    """Select the kernel kinds whose launches get HIP events (None = all)."""
    kinds = kernel_kinds()
    mask = 0xffffffff if names is None else sum(1 << kinds.index(x) for x in names)
    lib().bn254_set_profile_kernels(mask)


def set_rlc_params(min_batch=-1, adaptive=-1, share_min_lanes=-1):
    """Knobs of FLAG_RLC (bn254_set_rlc_params; -1 leaves a knob alone): batch size from which the flag is honoured, adaptive bypass, lanes a
    launch part must keep for shared Miller-loop accumulators."""
    lib().bn254_set_rlc_params(min_batch, adaptive, share_min_lanes)


def dbg_rlc_wide_plan(m, n_streams=2, log2_group=5, log2_share=3, min_lanes=65536, key_inputs=1024, msm_form=0):
    """Wide form of FLAG_RLC (keys with more than 8 inputs), bn254_dbg_g16_rlc_wide_plan: ({rows, digits, part}: bytes a context allocates for a chunk of m
    proofs, [(first group, groups)] per launch part as the enqueue places them)."""
    L = lib()
    L.bn254_dbg_g16_rlc_wide_plan.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                              C.c_int, C.POINTER(C.c_int)]
    alloc = (C.c_uint64 * 3)(); parts = (C.c_uint64 * 64)(); k = C.c_int()
    _check(L.bn254_dbg_g16_rlc_wide_plan(m, n_streams, log2_group, log2_share, min_lanes, key_inputs, msm_form, alloc, parts, 32, C.byref(k)))
    return {"rows": alloc[0], "digits": alloc[1], "part": alloc[2]}, [(parts[2 * i], parts[2 * i + 1]) for i in range(k.value)]


def dbg_rlc_groups(m):
    """The groups a chunk of m proofs forms under FLAG_RLC with the knobs as they stand (bn254_dbg_g16_rlc_groups: the plan the enqueue makes, host only).
    Returns (group of every proof, numbered through the chunk; log2 of the proofs per Miller-loop lane of every proof's launch part)."""
    L = lib()
    L.bn254_dbg_g16_rlc_groups.argtypes = [C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_uint8)]
    group = (C.c_uint * m)(); share = (C.c_uint8 * m)()
    _check(L.bn254_dbg_g16_rlc_groups(m, group, share))
    return list(group), list(share)


def dbg_overlap_replay(batches, fallback=True):
    """The stream-overlap decision over a sequence of batches, without a device (bn254_dbg_overlap_replay).  batches: per batch None (cannot be measured), "untimed"
    (measured, timings cannot be had) or (a0, a1, s1, e1) in ms.  Returns per batch (probe_now, single_stream, state, serial votes, last ratio read)."""
    L = lib()
    L.bn254_dbg_overlap_replay.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    n = len(batches)
    kind = bytes(0 if b is None else 2 if b == "untimed" else 1 for b in batches)
    timings = (C.c_float * (4 * n))(*[x for b in batches for x in (b if isinstance(b, tuple) else (0, 0, 0, 0))])
    out = (C.c_int * (4 * n))(); ratio = (C.c_float * n)()
    _check(L.bn254_dbg_overlap_replay(kind, timings, n, 1 if fallback else 0, out, ratio))
    return [(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3], ratio[i]) for i in range(n)]


def dbg_rlc_wide_group(kpts, alpha, weights, live, inputs, n_public, n, log2_group=5, log2_share=0, group=0):
    """Host compile of the wide FLAG_RLC group stage (bn254_dbg_rlc_wide_group).  kpts: K_0 .. K_n_public (64-byte uncompressed each, concatenated), alpha: 64 bytes,
    weights: 16 bytes per proof (k1, k2 little-endian u64), live: n bytes, inputs: n x n_public x 32 bytes.  Returns (per group a list of n_public 32-byte scalars
    sum r_i x_ij mod r, the uncompressed point t_0 K_0 + sum_j s_j K_j of group `group`, 64 zero bytes for the identity)."""
    L = lib()
    L.bn254_dbg_rlc_wide_group.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_uint, C.c_void_p,
                                           C.POINTER(C.c_uint), C.c_void_p]
    groups = C.c_uint()
    _check(L.bn254_dbg_rlc_wide_group(None, None, None, None, None, n_public, n, log2_group, log2_share, 0, None, C.byref(groups), None))
    g = groups.value
    out = (C.c_uint8 * max(1, g * n_public * 32))(); lo = (C.c_uint8 * 64)()
    _check(L.bn254_dbg_rlc_wide_group(bytes(kpts), bytes(alpha), bytes(weights), bytes(live), bytes(inputs) if n_public else None, n_public, n, log2_group, log2_share,
                                      group, out, C.byref(groups), lo))
    raw = bytes(out)
    return [[raw[(gi * n_public + j) * 32:(gi * n_public + j + 1) * 32] for j in range(n_public)] for gi in range(g)], bytes(lo)


def set_plonk_params(piece=-1, workers=-1, big_from=-1, big_piece=-1):
    """Knobs of the PlonK batch plan (bn254_set_plonk_params; -1 leaves a knob alone)."""
    L = lib()
    L.bn254_set_plonk_params.argtypes = [C.c_long, C.c_int, C.c_long, C.c_long]
    L.bn254_set_plonk_params.restype = None
    L.bn254_set_plonk_params(piece, workers, big_from, big_piece)


def set_keys_params(coop_max=-1):
    """Knob of the plan of a batch over many keys (bn254_set_keys_params): batches of up to coop_max proofs take the direct cooperative form, larger ones the grouped
    lane form; 0: always grouped; a negative value leaves the knob alone."""
    L = lib()
    L.bn254_set_keys_params.argtypes = [C.c_long]
    L.bn254_set_keys_params.restype = None
    L.bn254_set_keys_params(coop_max)


def dbg_keys_plan(n, n_keys):
    """The plan of a batch of n proofs over n_keys keys (bn254_dbg_g16_keys_plan): (form, slots, launches) -- form 0: grouped lanes, 1: direct cooperative."""
    L = lib()
    L.bn254_dbg_g16_keys_plan.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    form, slots, launches = C.c_int(-1), C.c_size_t(0), C.c_int(0)
    _check(L.bn254_dbg_g16_keys_plan(n, n_keys, C.byref(form), C.byref(slots), C.byref(launches)))
    return int(form.value), int(slots.value), int(launches.value)


def _check(rc):
    if rc != 0:
        e = (Bn254SelfTestError if rc == E_SELFTEST else Bn254Error)("bn254 error %d: %s" % (rc, lib().bn254_last_error().decode()))
        e.code = rc
        raise e


def selftest_check_names():
    L = lib()
    L.bn254_selftest_check_name.restype = C.c_char_p
    return [L.bn254_selftest_check_name(k).decode() for k in range(SELFTEST_NUM_CHECKS)]


def device_selftest(device=0):
    """The known-answer self-test of the verdict kernels on `device`, now (bn254_device_selftest): {"passed", "failed": names of the checks that disagree, "mask", "ms",
    "error": the library's text for the first failing check or None}.  The result replaces the device's recorded state.  Raises for everything but a failed check
    (no device, out of memory, ..)."""
    L = lib()
    mask, ms = C.c_uint(0), C.c_float(0)
    rc = L.bn254_device_selftest(int(device), C.byref(mask), C.byref(ms))
    if rc != 0 and rc != E_SELFTEST:
        _check(rc)
    names = selftest_check_names()
    return {"passed": rc == 0, "failed": [names[k] for k in range(SELFTEST_NUM_CHECKS) if mask.value >> k & 1], "mask": int(mask.value), "ms": float(ms.value),
            "error": L.bn254_last_error().decode() if rc else None}


def selftest_state(device=0):
    """(state, failed mask) of the device's recorded self-test (bn254_device_selftest_state): -1 not run yet, 0 failed, 1 passed, 2 skipped (BN254_SELFTEST=0)."""
    state, mask = C.c_int(-1), C.c_uint(0)
    _check(lib().bn254_device_selftest_state(int(device), C.byref(state), C.byref(mask)))
    return int(state.value), int(mask.value)


def dbg_selftest(device=0, corrupt_check=-1, record=False):
    """bn254_dbg_selftest: the self-test with one bit of check corrupt_check's device-side input flipped (-1: none): (return code, failed mask, error text)."""
    L = lib()
    mask = C.c_uint(0)
    rc = L.bn254_dbg_selftest(int(device), int(corrupt_check), 1 if record else 0, C.byref(mask))
    return rc, int(mask.value), L.bn254_last_error().decode() if rc else ""


def _inputs_bytes(public_inputs):
    return b"".join(x if isinstance(x, (bytes, bytearray)) else int(x).to_bytes(32, "big") for x in public_inputs)


class PreparedPlonkVk:
    """Opaque prepared PlonK verifying key (bn254_plonk_vk_prepare)."""

    def __init__(self, vk_bytes):
        self._h = C.c_void_p()
        _check(lib().bn254_plonk_vk_prepare(bytes(vk_bytes), len(vk_bytes), C.byref(self._h)))
        self.n_public = lib().bn254_plonk_vk_num_public(self._h)

    def verify_batch(self, proofs, public_inputs, n=None, proof_stride=904, n_public=None, device=0, flags=0):
        """proofs: n * proof_stride bytes; public_inputs: n * n_public * 32 bytes.  Returns n status bytes.  flags: FLAG_RLC batches the pairing checks of a pass across
        proofs (honoured from 8192 proofs per pass; exact fallback on the groups that fail)."""
        n_public = self.n_public if n_public is None else n_public
        if n is None:
            n = len(proofs) // proof_stride
        st = (C.c_uint8 * max(n, 1))()
        _check(lib().bn254_plonk_verify_batch_flags(self._h, bytes(proofs), proof_stride, bytes(public_inputs), n_public, n, st, device, flags))
        return bytes(st)[:n]

    def verify_batch_multi(self, proofs, public_inputs, device_mask, n=None, proof_stride=904, n_public=None, flags=0):
        """Same over the GPUs selected by the bits of device_mask (contiguous shards, one host thread per device)."""
        n_public = self.n_public if n_public is None else n_public
        if n is None:
            n = len(proofs) // proof_stride
        st = (C.c_uint8 * max(n, 1))()
        _check(lib().bn254_plonk_verify_batch_multi(self._h, bytes(proofs), proof_stride, bytes(public_inputs), n_public, n, st, device_mask, flags))
        return bytes(st)[:n]

    def verify_batch_device(self, d_proofs, d_inputs, d_status, n, proof_stride=904, n_public=None, device=0, stream=None, flags=0):
        """Raw device pointers (ints).  Host-synchronous: waits for `stream`, returns when the status bytes are in d_status."""
        n_public = self.n_public if n_public is None else n_public
        _check(lib().bn254_plonk_verify_batch_device(self._h, d_proofs, proof_stride, d_inputs, n_public, n, d_status, device, stream, flags))

    def verify_sp1_batch(self, proofs, vkey_hashes, public_values, proof_stride=904, device=0, flags=0):
        """SP1 proofs from their public values (bn254_sp1_plonk_verify_batch): as PreparedVk.verify_sp1_batch; flags: FLAG_RLC only."""
        return _sp1_host_call(lib().bn254_sp1_plonk_verify_batch, self._h, proofs, proof_stride, vkey_hashes, public_values, len(public_values), device, flags)

    def verify_sp1_batch_device(self, d_proofs, d_vkey_hashes, d_public_values, pv_bytes, d_offsets, d_status, n, proof_stride=904, vkey_stride=32, device=0,
                                stream=None, flags=0):
        """Raw device pointers (ints).  Host-synchronous like verify_batch_device (bn254_sp1_plonk_verify_batch_device)."""
        fn = lib().bn254_sp1_plonk_verify_batch_device
        fn.argtypes = _SP1_DEVICE_ARGTYPES
        _check(fn(self._h, d_proofs, proof_stride, d_vkey_hashes, vkey_stride, d_public_values, pv_bytes, d_offsets, n, d_status, device, stream, flags))

    def reserve(self, n, proof_stride=0, device=0):
        """Allocate now what a batch of up to n proofs needs (proof_stride > 0: also the pinned staging of the host-buffer entry)."""
        _check(lib().bn254_plonk_reserve(self._h, n, proof_stride, device))

    def footprint(self, device=0):
        """(bytes of device memory this key's contexts hold on `device`, contexts that hold any)"""
        b, c = C.c_size_t(0), C.c_int(0)
        _check(lib().bn254_plonk_footprint(self._h, device, C.byref(b), C.byref(c)))
        return b.value, c.value

    def last_timing(self, device=0):
        """Stage and kernel durations (ms) of the first sub-batch of the last verify_batch (bn254_plonk_last_timing)."""
        ms = (C.c_float * 9)()
        lanes = (C.c_size_t * 2)()
        _check(lib().bn254_plonk_last_timing(self._h, device, ms, lanes))
        names = ("host_copy", "k_plonk_stage1", "k_g1_msm_rows_digest", "k_g1_sum_affine_digest", "k_plonk_stage2", "k_g1_msm_rows_kzg", "k_g1_sum_affine_kzg", "pairing_check", "sub_batch_wall")
        return dict(zip(names, ms)), (lanes[0], lanes[1])

    def close(self):
        if self._h:
            lib().bn254_plonk_vk_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlonkVerifier:
    """Mirror of the reference's `PlonkVerifier::verify(proof, vk, public_inputs)` (verifier/src/lib.rs:69-73): returns the
    status byte (ACCEPT or an error code; PlonK never answers REJECT)."""

    @staticmethod
    def verify(proof, vk, public_inputs):
        st = C.c_uint8(0xEE)
        ib = _inputs_bytes(public_inputs)
        _check(lib().bn254_plonk_verify(bytes(proof), len(proof), bytes(vk), len(vk), ib, len(ib) // 32, C.byref(st)))
        return st.value


def _g16_layout(flags, proof_stride, compressed):
    """(flags, proof_stride) of a Groth16 batch call: compressed=True sets FLAG_COMPRESSED_PROOFS; the default stride is that of the layout."""
    if compressed:
        flags |= FLAG_COMPRESSED_PROOFS
    if proof_stride is None:
        proof_stride = COMPRESSED_PROOF_LEN if flags & FLAG_COMPRESSED_PROOFS else 256
    return flags, proof_stride


def compress_proof(raw):
    """gnark's compressed form (128 bytes) of a raw Groth16 proof A (64) | B (128) | C (64): bn254_g1_compress / bn254_g2_compress of the three points."""
    L = lib()
    raw = bytes(raw)
    a, b, c = (C.c_uint8 * 32)(), (C.c_uint8 * 64)(), (C.c_uint8 * 32)()
    _check(L.bn254_g1_compress(raw[0:64], a))
    _check(L.bn254_g2_compress(raw[64:192], b))
    _check(L.bn254_g1_compress(raw[192:256], c))
    return bytes(a) + bytes(b) + bytes(c)


def dbg_g16_decompress(records, k=None, stride=COMPRESSED_PROOF_LEN):
    """Host compile of k_g16_decompress's body (bn254_dbg_g16_decompress): (k raw 256-byte records, k pre-status bytes: 0 decompressed, 1 MALFORMED)."""
    L = lib()
    L.bn254_dbg_g16_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    records = bytes(records)
    if k is None:
        k = len(records) // stride
    raw = (C.c_uint8 * max(1, 256 * k))(); pre = (C.c_uint8 * max(1, k))()
    _check(L.bn254_dbg_g16_decompress(records, stride, k, raw, pre))
    return bytes(raw)[:256 * k], bytes(pre)[:k]


def sp1_public_values_digest(public_values):
    """SP1's committed_values_digest: SHA-256(public_values) with the top three bits of byte 0 cleared (bn254_sp1_public_values_digest, on the host)."""
    L = lib()
    L.bn254_sp1_public_values_digest.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    out = (C.c_uint8 * 32)()
    pv = bytes(public_values)
    _check(L.bn254_sp1_public_values_digest(pv, len(pv), out))
    return bytes(out)


def sp1_pack_values(public_values, base=0):
    """A list of byte strings -> (their concatenation, the n + 1 absolute offsets of the SP1 entries as a ctypes uint64 array; the first is `base`)."""
    import numpy as np
    vals = public_values if all(isinstance(v, bytes) for v in public_values) else [bytes(v) for v in public_values]
    offs = (C.c_uint64 * (len(vals) + 1))()
    o = np.frombuffer(offs, dtype=np.uint64)
    o[0] = base
    np.cumsum(np.fromiter(map(len, vals), dtype=np.uint64, count=len(vals)), out=o[1:])
    o[1:] += np.uint64(base)
    return b"".join(vals), offs


def _sp1_vkey_hashes(vkey_hashes, n):
    """One 32-byte hash for the whole batch (stride 0) or a list of n (stride 32) -> (bytes, stride)."""
    if isinstance(vkey_hashes, (bytes, bytearray)):
        if len(vkey_hashes) != 32:
            raise ValueError("one vkey hash is 32 bytes; pass a list for one hash per proof")
        return bytes(vkey_hashes), 0
    hs = [bytes(h) for h in vkey_hashes]
    if len(hs) != n or any(len(h) != 32 for h in hs):
        raise ValueError("vkey_hashes: one 32-byte hash, or n of them")
    return b"".join(hs), 32


def _offsets_ptr(offsets):
    """A ctypes uint64 array, or an int (a device pointer)."""
    return offsets if isinstance(offsets, int) else C.cast(offsets, C.c_void_p)


def dbg_sp1_public_inputs(vkey_hashes, vkey_stride, public_values, offsets, n=None, pv_bytes=None, device=-1):
    """k_sp1_public_inputs's body (bn254_dbg_sp1_public_inputs) on host buffers: device -1 runs the host compile, device >= 0 the kernel.  offsets: n + 1
    integers.  Returns (n rows of 64 bytes vkey_hash | digest, n bad-range bytes)."""
    L = lib()
    L.bn254_dbg_sp1_public_inputs.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    offs = list(offsets)
    if n is None:
        n = len(offs) - 1
    pv = bytes(public_values)
    pv_bytes = len(pv) if pv_bytes is None else pv_bytes
    oa = (C.c_uint64 * max(1, len(offs)))(*offs)
    rows = (C.c_uint8 * max(1, 64 * n))(); bad = (C.c_uint8 * max(1, n))()
    _check(L.bn254_dbg_sp1_public_inputs(bytes(vkey_hashes), vkey_stride, pv, pv_bytes, C.cast(oa, C.c_void_p), n, rows, bad, device))
    return bytes(rows)[:64 * n], bytes(bad)[:n]


def synth_groth16_for_inputs(seed, n_public, inputs, n=None, threads=0):
    """(vk, proofs): the key of synth_groth16(seed, n_public, ..) and one valid 256-byte proof per input row (n x n_public x 32 bytes, used modulo r)."""
    L = lib()
    L.bn254_synth_groth16_for_inputs.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    inputs = bytes(inputs)
    if n is None:
        n = len(inputs) // (32 * n_public)
    vk = (C.c_uint8 * L.bn254_synth_groth16_vk_len(n_public))()
    proofs = (C.c_uint8 * max(256 * n, 1))()
    _check(L.bn254_synth_groth16_for_inputs(seed, n_public, n, inputs, threads, vk, proofs))
    return bytes(vk), bytes(proofs)[:256 * n]


def _sp1_host_call(fn, handle, proofs, proof_stride, vkey_hashes, public_values, n, device, flags):
    vk, vstride = _sp1_vkey_hashes(vkey_hashes, n)
    pv, offs = sp1_pack_values(public_values)
    st = (C.c_uint8 * max(n, 1))()
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    _check(fn(handle, bytes(proofs), proof_stride, vk, vstride, pv, C.cast(offs, C.c_void_p), n, st, device, flags))
    return bytes(st)[:n]


_SP1_DEVICE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]


class PreparedVk:
    """Opaque prepared verifying key (bn254_groth16_vk_prepare)."""

    def __init__(self, vk_bytes, mode=VK_REFERENCE):
        self._h = C.c_void_p()
        _check(lib().bn254_groth16_vk_prepare(bytes(vk_bytes), len(vk_bytes), mode, C.byref(self._h)))
        self.n_public = lib().bn254_groth16_vk_num_public(self._h)

    @property
    def handle(self):
        return self._h

    def verify_batch(self, proofs, public_inputs, n=None, proof_stride=None, n_public=None, device=0, flags=0, compressed=False):
        """proofs: bytes (n * proof_stride); public_inputs: bytes (n * n_public * 32). Returns n status bytes.
        flags: FLAG_STRICT_SCALARS | FLAG_RLC (include/bn254_verify.h).  compressed: the records are gnark's compressed proofs (FLAG_COMPRESSED_PROOFS;
        proof_stride defaults to 128 then, 256 otherwise)."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        n_public = self.n_public if n_public is None else n_public
        if n is None:
            n = len(proofs) // proof_stride
        st = (C.c_uint8 * max(n, 1))()
        _check(lib().bn254_groth16_verify_batch(self._h, bytes(proofs), proof_stride, bytes(public_inputs), n_public, n, st, device, flags))
        return bytes(st)[:n]

    def verify_batch_multi(self, proofs, public_inputs, device_mask, n=None, proof_stride=None, n_public=None, flags=0, compressed=False):
        """Same over the GPUs selected by the bits of device_mask (contiguous shards, one host thread per device)."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        n_public = self.n_public if n_public is None else n_public
        if n is None:
            n = len(proofs) // proof_stride
        st = (C.c_uint8 * max(n, 1))()
        _check(lib().bn254_groth16_verify_batch_multi(self._h, bytes(proofs), proof_stride, bytes(public_inputs), n_public, n, st, device_mask, flags))
        return bytes(st)[:n]

    def verify_batch_device(self, d_proofs, d_inputs, d_status, n, proof_stride=None, n_public=None, device=0, stream=None, flags=0, compressed=False):
        """Raw device pointers (ints); enqueues on `stream` (a hipStream_t value) and returns (FLAG_RLC: after one stream sync)."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        n_public = self.n_public if n_public is None else n_public
        _check(lib().bn254_groth16_verify_batch_device(self._h, d_proofs, proof_stride, d_inputs, n_public, n, d_status, device, stream, flags))

    def verify_sp1_batch(self, proofs, vkey_hashes, public_values, proof_stride=None, device=0, flags=0, compressed=False):
        """SP1 proofs from their public values (bn254_sp1_groth16_verify_batch): proofs as verify_batch takes them (n records); vkey_hashes: one 32-byte
        hash or a list of n; public_values: a list of n byte strings.  The inputs vkey_hash | SHA-256(values) & mask are made on the device.  Returns n status bytes."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        return _sp1_host_call(lib().bn254_sp1_groth16_verify_batch, self._h, proofs, proof_stride, vkey_hashes, public_values, len(public_values), device, flags)

    def verify_sp1_batch_device(self, d_proofs, d_vkey_hashes, d_public_values, pv_bytes, d_offsets, d_status, n, proof_stride=None, vkey_stride=32, device=0,
                                stream=None, flags=0, compressed=False):
        """Raw device pointers (ints; d_offsets: n + 1 uint64 values); enqueues on `stream` like verify_batch_device (bn254_sp1_groth16_verify_batch_device)."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        fn = lib().bn254_sp1_groth16_verify_batch_device
        fn.argtypes = _SP1_DEVICE_ARGTYPES
        _check(fn(self._h, d_proofs, proof_stride, d_vkey_hashes, vkey_stride, d_public_values, pv_bytes, d_offsets, n, d_status, device, stream, flags))

    def reserve(self, n, device=0):
        _check(lib().bn254_groth16_reserve(self._h, n, device))

    def rlc_state(self, device=0):
        """(share of the checked proofs the recent FLAG_RLC passes sent to the exact fallback, -1.0 before the first pass; calls that bypassed the mode)."""
        share, by = C.c_float(), C.c_uint()
        _check(lib().bn254_groth16_rlc_state(self._h, device, C.byref(share), C.byref(by)))
        return share.value, by.value

    def last_kernel_ms(self, device=0):
        ms = (C.c_float * NUM_KERNELS)()
        _check(lib().bn254_groth16_last_kernel_ms(self._h, device, ms))
        return {lib().bn254_groth16_kernel_name(i).decode(): ms[i] for i in range(NUM_KERNELS)}

    def kernel_profile(self, device=0):
        """Per kernel kind: {name: (launches, total_ms)} of the last profiled batch, and the proofs each launch covered."""
        k = lib().bn254_groth16_num_kernel_kinds()
        cnt = (C.c_uint * k)(); ms = (C.c_float * k)(); per = C.c_size_t(0)
        _check(lib().bn254_groth16_kernel_profile(self._h, device, cnt, ms, C.byref(per)))
        return {lib().bn254_groth16_kernel_kind_name(i).decode(): (int(cnt[i]), float(ms[i])) for i in range(k) if cnt[i]}, int(per.value)

    def kernel_profile_all(self, device=0):
        """Per kernel kind over the first two sub-batches (two streams): {name: (launches, total_ms, union_ms)}, and the proofs per launch."""
        k = lib().bn254_groth16_num_kernel_kinds()
        cnt = (C.c_uint * k)(); ms = (C.c_float * k)(); un = (C.c_float * k)(); per = C.c_size_t(0)
        _check(lib().bn254_groth16_kernel_profile_all(self._h, device, cnt, ms, un, C.byref(per)))
        return {lib().bn254_groth16_kernel_kind_name(i).decode(): (int(cnt[i]), float(ms[i]), float(un[i])) for i in range(k) if cnt[i]}, int(per.value)

    def close(self):
        if self._h:
            lib().bn254_groth16_vk_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _adopt_vk(handle):
    """A PreparedVk around a handle the library already made (prepare_vks)."""
    k = PreparedVk.__new__(PreparedVk)
    k._h = C.c_void_p(handle)
    k.n_public = lib().bn254_groth16_vk_num_public(k._h)
    return k


def _prepare_vks_call(fn, vks, mode, device, extra=()):
    vks = [bytes(v) for v in vks]
    n = len(vks)
    ptrs = (C.c_char_p * max(n, 1))(*vks)
    lens = (C.c_size_t * max(n, 1))(*[len(v) for v in vks])
    out = (C.c_void_p * max(n, 1))()
    status = (C.c_int * max(n, 1))()
    try:
        _check(fn(ptrs, lens, n, mode, device, out, status, *extra))
    except Exception:
        for h in out[:n]:
            if h:
                lib().bn254_groth16_vk_free(h)
        raise
    return [_adopt_vk(out[i]) if out[i] else None for i in range(n)], [int(status[i]) for i in range(n)]


def prepare_vks(vks, mode=VK_REFERENCE, device=0, with_status=False):
    """Many Groth16 verifying keys prepared in one call, on `device` (bn254_groth16_vk_prepare_batch): a list with a PreparedVk per key that loads and None per key
    that does not -- each handle equal to PreparedVk(vk, mode) in everything a caller can observe, independent of the others.  with_status: also the per-key return
    codes (0, or -4 for a key that does not load), as a second list."""
    fn = lib().bn254_groth16_vk_prepare_batch
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    keys, status = _prepare_vks_call(fn, vks, mode, device)
    return (keys, status) if with_status else keys


def dbg_prepare_vks(vks, mode=VK_REFERENCE, device=-1):
    """prepare_vks through the probe (bn254_dbg_g16_vk_prepare_batch): device -1 runs the kernels' bodies compiled for the host (csrc/bn254_vkprep.h) and touches no
    GPU.  Returns (keys, status, stage_ms) -- stage_ms: G1 decode, G2 decode, fold, line tables, pairing of the device passes, from HIP events."""
    fn = lib().bn254_dbg_g16_vk_prepare_batch
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ms = (C.c_float * 5)()
    keys, status = _prepare_vks_call(fn, vks, mode, device, (ms,))
    return keys, status, dict(zip(VK_PREPARE_STAGES, [float(x) for x in ms]))


VK_PREPARE_STAGES = ("k_vkp_dec_g1", "k_vkp_dec_g2", "k_vkp_fold", "k_vkp_lines", "pairing_program")


def dbg_pvk_image(key):
    """The host image of a prepared Groth16 key as bytes (bn254_dbg_g16_pvk_image): two handles of one key are interchangeable iff their images are equal."""
    fn = lib().bn254_dbg_g16_pvk_image
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    ln = C.c_size_t(0)
    fn(key.handle, None, 0, C.byref(ln))
    buf = (C.c_uint8 * max(ln.value, 1))()
    _check(fn(key.handle, buf, ln.value, C.byref(ln)))
    return bytes(buf)[:ln.value]


class KeySet:
    """A list of prepared Groth16 keys for batches over many keys (bn254_groth16_verify_batch_keys): proof i is verified against keys[key_index[i]].  keys: PreparedVk
    objects (one may occur more than once); the list keeps them alive.  Keys with more than 16 public inputs are refused by the library."""

    def __init__(self, keys):
        self.keys = list(keys)
        self._arr = (C.c_void_p * max(len(self.keys), 1))(*[k.handle.value for k in self.keys])
        self.input_stride = 32 * max([k.n_public for k in self.keys if k.n_public != C.c_size_t(-1).value] or [0])

    def _index(self, key_index):
        import array
        a = array.array("I", key_index)
        assert a.itemsize == 4
        return a

    def verify_batch(self, key_index, proofs, public_inputs, n=None, proof_stride=None, input_stride=None, device=0, flags=0, compressed=False):
        """key_index: n ints; proofs: n records; public_inputs: n rows of input_stride bytes (default: 32 x the largest input count of the list), row i holding the
        inputs of proof i's key first.  Returns n status bytes."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        idx = self._index(key_index)
        n = len(idx) if n is None else n
        st = (C.c_uint8 * max(n, 1))()
        fn = lib().bn254_groth16_verify_batch_keys
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
        _check(fn(self._arr, len(self.keys), idx.buffer_info()[0] if len(idx) else None, bytes(proofs), proof_stride, bytes(public_inputs),
                  self.input_stride if input_stride is None else input_stride, n, st, device, flags))
        return bytes(st)[:n]

    def verify_batch_device(self, d_key_index, d_proofs, d_inputs, d_status, n, proof_stride=None, input_stride=None, device=0, stream=None, flags=0, compressed=False):
        """Raw device pointers (ints; d_key_index: n uint32 values); enqueues on `stream` (a hipStream_t value) and returns."""
        flags, proof_stride = _g16_layout(flags, proof_stride, compressed)
        fn = lib().bn254_groth16_verify_batch_keys_device
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        _check(fn(self._arr, len(self.keys), d_key_index, d_proofs, proof_stride, d_inputs, self.input_stride if input_stride is None else input_stride, n, d_status, device,
                  stream, flags))

    def reserve(self, n, device=0):
        fn = lib().bn254_groth16_reserve_keys
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        _check(fn(self._arr, len(self.keys), n, device))

    def last_form(self, device=0):
        """Form of the last batch enqueued with this list on `device` (bn254_dbg_g16_keys_last_form): 0 grouped lanes, 1 direct cooperative, -1 none yet."""
        fn = lib().bn254_dbg_g16_keys_last_form
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
        form = C.c_int(-1)
        _check(fn(self._arr, len(self.keys), device, C.byref(form)))
        return int(form.value)


class PlonkKeySet:
    """A list of prepared PlonK keys for batches over many keys (bn254_plonk_verify_batch_keys): proof i is verified against keys[key_index[i]].  keys:
    PreparedPlonkVk objects (one may occur more than once; at most 256 entries, all with the same number of BSB22 commitments); the list keeps them alive."""

    def __init__(self, keys):
        self.keys = list(keys)
        self._arr = (C.c_void_p * max(len(self.keys), 1))(*[k._h.value for k in self.keys])
        self.input_stride = 32 * max([k.n_public for k in self.keys] or [0])

    def verify_batch(self, key_index, proofs, public_inputs, n=None, proof_stride=904, input_stride=None, device=0, flags=0):
        """key_index: n ints; proofs: n records of proof_stride bytes; public_inputs: n rows of input_stride bytes (default: 32 x the largest input count of the
        list), row i holding the inputs of proof i's key first.  Returns n status bytes."""
        import array
        idx = array.array("I", key_index)
        n = len(idx) if n is None else n
        st = (C.c_uint8 * max(n, 1))()
        fn = lib().bn254_plonk_verify_batch_keys
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
        _check(fn(self._arr, len(self.keys), idx.buffer_info()[0] if len(idx) else None, bytes(proofs), proof_stride, bytes(public_inputs) if public_inputs is not None else None,
                  self.input_stride if input_stride is None else input_stride, n, st, device, flags))
        return bytes(st)[:n]

    def verify_batch_device(self, d_key_index, d_proofs, d_inputs, d_status, n, proof_stride=904, input_stride=None, device=0, stream=None, flags=0):
        """Raw device pointers (ints; d_key_index: n uint32 values).  Host-synchronous: waits for `stream`, returns when the status bytes are in d_status."""
        fn = lib().bn254_plonk_verify_batch_keys_device
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        _check(fn(self._arr, len(self.keys), d_key_index, d_proofs, proof_stride, d_inputs, self.input_stride if input_stride is None else input_stride, n, d_status, device,
                  stream, flags))

    def reserve(self, n, proof_stride=904, device=0):
        fn = lib().bn254_plonk_reserve_keys
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        _check(fn(self._arr, len(self.keys), n, proof_stride, device))


    def state(self, device=0):
        """Counters of this list's cached state on `device` since the state was created (bn254_plonk_keys_state): (passes that ran the joint check of FLAG_RLC, groups
        they checked, groups that failed, passes whose per-proof pairing check ran in the cooperative form).  Raises if the list is not cached."""
        fn = lib().bn254_plonk_keys_state
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
        out = (C.c_uint64 * 4)()
        _check(fn(self._arr, len(self.keys), device, out))
        return tuple(int(v) for v in out)

    def dbg_coop12_miller_fixed(self, key_words, key_shift, g1_0, g1_1, identity=None, n=None, device=0):
        """The cooperative two-pair check with the key per item in store mode (bn254_dbg_coop12_miller_fixed_keys): item i belongs to keys[key_words[i >> key_shift]];
        g1_0 / g1_1: n affine G1 points of 64 bytes; identity: None or n bytes (bit 0 / 1: pair 0 / 1 is the identity).  Returns n values of 384 bytes."""
        import array
        n = len(g1_0) // 64 if n is None else n
        kw = array.array("I", key_words)
        fn = lib().bn254_dbg_coop12_miller_fixed_keys
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
        out = (C.c_uint8 * (384 * max(n, 1)))()
        _check(fn(self._arr, len(self.keys), kw.buffer_info()[0] if len(kw) else None, key_shift, bytes(g1_0), bytes(g1_1), bytes(identity) if identity is not None else None, out, n, device))
        raw = bytes(out)
        return [raw[384 * i:384 * (i + 1)] for i in range(n)]


def set_plonk_keys_params(coop_max=-1):
    """bn254_set_plonk_keys_params: passes of up to coop_max slots of a PlonK batch over a key list take the cooperative pairing form (0: always the lane form; clamped
    to the cooperative kernel's range; negative: unchanged)."""
    fn = lib().bn254_set_plonk_keys_params
    fn.argtypes = [C.c_long]; fn.restype = None
    fn(coop_max)


def set_plonk_rlc_params(min_pass=-1):
    """bn254_set_plonk_rlc_params: the pass size from which the PlonK entries honour FLAG_RLC (one key and key lists; never below 64; negative: unchanged)."""
    fn = lib().bn254_set_plonk_rlc_params
    fn.argtypes = [C.c_long]; fn.restype = None
    fn(min_pass)


def dbg_plonk_keys_knobs():
    """(coop_max, rlc_min_pass) as they are now (bn254_dbg_plonk_keys_knobs)."""
    fn = lib().bn254_dbg_plonk_keys_knobs
    fn.argtypes = [C.POINTER(C.c_long)]
    out = (C.c_long * 2)()
    _check(fn(out))
    return int(out[0]), int(out[1])


def dbg_plonk_keys_plan(n, n_keys, slots):
    """The plan of a PlonK batch over many keys (bn254_dbg_plonk_keys_plan): dict with slot_bound, workers, per_worker, per_pass, ctx_capacity and pass_first."""
    fn = lib().bn254_dbg_plonk_keys_plan
    P = C.POINTER(C.c_size_t)
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, P, C.POINTER(C.c_int), P, P, P, P, C.c_size_t, P]
    bound, per, pas, cap, np_ = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    w = C.c_int(0)
    first = (C.c_size_t * 8192)()
    _check(fn(n, n_keys, slots, C.byref(bound), C.byref(w), C.byref(per), C.byref(pas), C.byref(cap), first, 8192, C.byref(np_)))
    assert np_.value <= 8192
    return dict(slot_bound=bound.value, workers=w.value, per_worker=per.value, per_pass=pas.value, ctx_capacity=cap.value, pass_first=list(first[:np_.value]))


def last_diagnostic():
    """bn254_last_diagnostic() of the calling thread."""
    lib().bn254_last_diagnostic.restype = C.c_char_p
    return (lib().bn254_last_diagnostic() or b"").decode()


def dbg_keys_group(key_index, n_keys, device=-1):
    """The grouping of a batch over many keys (bn254_dbg_g16_keys_group; device -1: the host compile of csrc/bn254_keys.h): (slot_to_proof, granule_key, n_slots) --
    slot_to_proof has the workspace bound's length (0xffffffff: no proof), granule_key one entry per 64 slots."""
    import array
    L = lib()
    L.bn254_dbg_g16_keys_slot_bound.argtypes = [C.c_size_t, C.c_size_t]; L.bn254_dbg_g16_keys_slot_bound.restype = C.c_size_t
    L.bn254_dbg_g16_keys_group.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    idx = array.array("I", key_index)
    bound = L.bn254_dbg_g16_keys_slot_bound(len(idx), n_keys)
    s2p = array.array("I", bytes(4 * bound)); gk = array.array("I", bytes(4 * (bound // 64)))
    ns = C.c_size_t(0)
    _check(L.bn254_dbg_g16_keys_group(idx.buffer_info()[0], len(idx), n_keys, device, s2p.buffer_info()[0], gk.buffer_info()[0] if len(gk) else None, C.byref(ns)))
    return s2p, gk, int(ns.value)


class Groth16Verifier:
    """Mirror of the reference's `Groth16Verifier` (verifier/src/lib.rs:29-49)."""

    @staticmethod
    def verify(proof, vk, public_inputs, mode=VK_REFERENCE):
        """Returns the status byte: ACCEPT = Ok(true), REJECT = Ok(false), ERR_INPUT_LEN = Err(PrepareInputsFailed);
        the other ERR_* codes are the reference's panics (unwrap of a loader error)."""
        st = C.c_uint8(0xEE)
        ib = _inputs_bytes(public_inputs)
        _check(lib().bn254_groth16_verify(bytes(proof), len(proof), bytes(vk), len(vk), ib, len(public_inputs), mode, C.byref(st)))
        return st.value

    @staticmethod
    def verify_batch(proofs, vk, public_inputs, mode=VK_REFERENCE, device=0):
        """proofs: list of byte strings; public_inputs: list of lists. Returns a list of status bytes."""
        pvk = PreparedVk(vk, mode)
        try:
            n = len(proofs)
            stride = max([256] + [len(p) for p in proofs])
            pb = b"".join(bytes(p).ljust(stride, b"\0") for p in proofs)
            npub = len(public_inputs[0]) if n else 0
            ib = b"".join(_inputs_bytes(x) for x in public_inputs)
            short = [len(p) < 256 for p in proofs]
            st = list(pvk.verify_batch(pb, ib, n, stride, npub, device))
            return [ERR_MALFORMED if s else v for s, v in zip(short, st)]
        finally:
            pvk.close()


def proof_write_raw(a, b, c):
    """The 324-byte raw gnark proof (A | B | C | no commitments | zero PoK) that groth16/converter.rs:14-26 reads."""
    out = (C.c_uint8 * RAW_PROOF_LEN)()
    _check(lib().bn254_groth16_proof_write_raw(bytes(a), bytes(b), bytes(c), out))
    return bytes(out)


def shard_plan(n, device_mask, device_count):
    """[(device, first, count)] of bn254_groth16_verify_batch_multi's shards (bn254_shard_plan: host arithmetic, no GPU)."""
    devs = (C.c_int * 64)(); first = (C.c_size_t * 64)(); cnt = (C.c_size_t * 64)(); k = C.c_int(0)
    _check(lib().bn254_shard_plan(n, device_mask, device_count, devs, first, cnt, C.byref(k)))
    return [(devs[i], first[i], cnt[i]) for i in range(k.value)]


def synth_groth16(seed, n_public, n, invalid_every=16, agree=True, threads=0, l_identity=False, first=0):
    """Deterministic synthetic gnark-format workload: (vk, proofs, inputs, expected_status) as bytes.  first: global index of the first
    proof (proof i of the stream depends on (seed, i) only, so a rank can generate its own shard)."""
    L = lib()
    vk = (C.c_uint8 * L.bn254_synth_groth16_vk_len(n_public))()
    proofs = (C.c_uint8 * max(256 * n, 1))()
    inputs = (C.c_uint8 * max(32 * n_public * n, 1))()
    exp = (C.c_uint8 * max(n, 1))()
    # l_identity: every proof with index = 3 mod 7 gets public inputs that make its public-input point L the identity (a valid proof)
    _check(L.bn254_synth_groth16_range(seed, n_public, first, n, invalid_every, (1 if agree else 0) | (2 if l_identity else 0), threads, vk, proofs, inputs, exp))
    return bytes(vk), bytes(proofs)[:256 * n], bytes(inputs)[:32 * n_public * n], bytes(exp)[:n]


def _synth_plonk_lib():
    L = lib()
    L.bn254_synth_plonk_vk_len.restype = C.c_size_t; L.bn254_synth_plonk_vk_len.argtypes = [C.c_size_t]
    L.bn254_synth_plonk_proof_len.restype = C.c_size_t; L.bn254_synth_plonk_proof_len.argtypes = [C.c_size_t]
    L.bn254_synth_plonk_range.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p]
    L.bn254_synth_plonk_for_inputs.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def synth_plonk(seed, n_public, n_qcp, log2_size, n, invalid_every=16, threads=0, first=0, proof_stride=None):
    """Deterministic synthetic PlonK workload for a key with n_public inputs, n_qcp BSB22 commitments and 2^log2_size rows: (vk, proofs, inputs, expected_status)
    as bytes, the proofs all distinct and proof_stride bytes apart (default: the proof length, 808 + 96 n_qcp).  first: global index of the first proof (proof i
    of the stream depends on (seed, i) and the key only)."""
    L = _synth_plonk_lib()
    if n_qcp > 8:
        raise Bn254Error("bn254_synth_plonk: at most 8 commitments")
    stride = L.bn254_synth_plonk_proof_len(n_qcp) if proof_stride is None else proof_stride
    vk = (C.c_uint8 * L.bn254_synth_plonk_vk_len(n_qcp))()
    proofs = (C.c_uint8 * max(stride * n, 1))()
    inputs = (C.c_uint8 * max(32 * n_public * n, 1))()
    exp = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_synth_plonk_range(seed, n_public, n_qcp, log2_size, first, n, invalid_every, threads, vk, proofs, stride, inputs, exp))
    return bytes(vk), bytes(proofs)[:stride * n], bytes(inputs)[:32 * n_public * n], bytes(exp)[:n]


def synth_plonk_for_inputs(seed, n_public, n_qcp, log2_size, inputs, n=None, threads=0, proof_stride=None):
    """(vk, proofs): the key of synth_plonk for the same arguments and one valid proof per input row (n x n_public x 32 bytes, each value below r)."""
    L = _synth_plonk_lib()
    if n_qcp > 8:
        raise Bn254Error("bn254_synth_plonk_for_inputs: at most 8 commitments")
    inputs = bytes(inputs)
    if n is None:
        n = len(inputs) // (32 * n_public)
    stride = L.bn254_synth_plonk_proof_len(n_qcp) if proof_stride is None else proof_stride
    vk = (C.c_uint8 * L.bn254_synth_plonk_vk_len(n_qcp))()
    proofs = (C.c_uint8 * max(stride * n, 1))()
    _check(L.bn254_synth_plonk_for_inputs(seed, n_public, n_qcp, log2_size, n, inputs, threads, vk, proofs, stride))
    return bytes(vk), bytes(proofs)[:stride * n]


PLONK_STAGES_REC = 560


def _plonk_stage_records(raw, n):
    """The records of bn254_dbg_plonk_stages (include/bn254_verify.h has the layout) as dicts of bytes / ints."""
    out = []
    for i in range(n):
        r = raw[PLONK_STAGES_REC * i:PLONK_STAGES_REC * (i + 1)]
        out.append({"status1": r[0], "status": r[1], "lin_inf": r[2], "p0_inf": r[3], "p1_inf": r[4], "slot": int.from_bytes(r[8:12], "little"), "zeta": r[16:48],
                    "lambda": r[48:80], "lin_opening": r[80:112], "lin": r[112:176], "h2f": [r[176 + 32 * k:208 + 32 * k] for k in range(8)],
                    "p0": r[432:496], "p1": r[496:560], "pad": r[5:8] + r[12:16]})
    return out


def dbg_plonk_stages(key, proofs, public_inputs, lam_key, n=None, proof_stride=904, n_public=None, flags=0, device=0):
    """bn254_dbg_plonk_stages: the product's pass up to the pairing operands on n <= 4096 proofs under the caller's ChaCha20 key (lam_key: 11 ints below 2^32).
    key: a PreparedPlonkVk.  device -1: the host compile of the stages, no device.  Returns one dict per proof ("h2f": all eight values, those past the key's
    commitment count zero)."""
    n_public = key.n_public if n_public is None else n_public
    if n is None:
        n = len(proofs) // proof_stride
    fn = lib().bn254_dbg_plonk_stages
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint, C.c_void_p, C.c_int]
    out = (C.c_uint8 * (PLONK_STAGES_REC * max(n, 1)))()
    lk = (C.c_uint32 * 11)(*lam_key) if lam_key is not None else None
    _check(fn(key._h if key is not None else None, bytes(proofs) if proofs is not None else None, proof_stride, bytes(public_inputs) if public_inputs is not None else None,
              n_public, n, lk, flags, out, device))
    return _plonk_stage_records(bytes(out), n)


def dbg_plonk_stages_keys(key_set, key_index, proofs, public_inputs, lam_key, n=None, proof_stride=904, input_stride=None, flags=0, device=0):
    """bn254_dbg_plonk_stages_keys: the same over a PlonkKeySet, through the gather of a batch over many keys; a record's "slot" is the slot the grouping gave the
    proof (lambda and the weight are drawn per slot)."""
    import array
    idx = array.array("I", key_index)
    n = len(idx) if n is None else n
    fn = lib().bn254_dbg_plonk_stages_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint, C.c_void_p, C.c_int]
    out = (C.c_uint8 * (PLONK_STAGES_REC * max(n, 1)))()
    lk = (C.c_uint32 * 11)(*lam_key) if lam_key is not None else None
    _check(fn(key_set._arr, len(key_set.keys), idx.buffer_info()[0] if len(idx) else None, bytes(proofs), proof_stride, bytes(public_inputs) if public_inputs is not None else None,
              key_set.input_stride if input_stride is None else input_stride, n, lk, flags, out, device))
    return _plonk_stage_records(bytes(out), n)


# ---- batch pairing-product checks over caller-supplied (G1, G2) pairs (bn254_pairing_check_batch, include/bn254_verify.h) ----
PAIRING_MAX_PAIRS = 8
PAIRING_PAIR_LEN = 192


def _pairing_lib():
    L = lib()
    host = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t]
    L.bn254_pairing_check_batch.argtypes = host + [C.c_void_p, C.c_int]
    L.bn254_pairing_batch.argtypes = host + [C.c_void_p, C.c_void_p, C.c_int]
    L.bn254_dbg_pairing_batch.argtypes = host + [C.c_void_p, C.c_void_p, C.c_int]
    L.bn254_pairing_check_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.bn254_pairing_reserve.argtypes = [C.c_size_t, C.c_int]
    L.bn254_dbg_pairing_plan.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
    return L


def _pairing_shape(pairs, n_pairs, n, item_stride):
    pairs = bytes(pairs)
    if item_stride is None:
        item_stride = PAIRING_PAIR_LEN * n_pairs
    if n is None:
        n = len(pairs) // item_stride if item_stride else 0
    if n and len(pairs) < (n - 1) * item_stride + PAIRING_PAIR_LEN * n_pairs:
        raise Bn254Error("pairing batch: the buffer is shorter than n items")
    return pairs, n, item_stride


def pairing_check_batch(pairs, n_pairs, n=None, item_stride=None, device=0):
    """n items of n_pairs records G1 (64) | G2 (128: x.c1 | x.c0 | y.c1 | y.c0), item_stride bytes apart -> n status bytes: ACCEPT where the product of the item's
    pairings is 1, REJECT where it is not, or the loader error (bn254_pairing_check_batch; EIP-197's ecPairing per item)."""
    L = _pairing_lib()
    pairs, n, item_stride = _pairing_shape(pairs, n_pairs, n, item_stride)
    status = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_pairing_check_batch(pairs, item_stride, n_pairs, n, status, device))
    return bytes(status)[:n]


def pairing_batch(pairs, n_pairs, n=None, item_stride=None, device=0):
    """(n GT values of 384 bytes -- the final-exponentiated product of each item's pairings, tower order -- and n status bytes: ACCEPT where the value is valid,
    else the loader error)  (bn254_pairing_batch)."""
    L = _pairing_lib()
    pairs, n, item_stride = _pairing_shape(pairs, n_pairs, n, item_stride)
    gt = (C.c_uint8 * max(384 * n, 1))(); status = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_pairing_batch(pairs, item_stride, n_pairs, n, gt, status, device))
    return bytes(gt)[:384 * n], bytes(status)[:n]


def pairing_check_batch_device(d_pairs, n_pairs, n, d_status, item_stride=None, device=0, stream=0):
    """bn254_pairing_check_batch_device on device pointers (ints): enqueues on `stream` (a hipStream_t as int) and returns; the caller synchronises the stream."""
    L = _pairing_lib()
    _check(L.bn254_pairing_check_batch_device(d_pairs, PAIRING_PAIR_LEN * n_pairs if item_stride is None else item_stride, n_pairs, n, d_status, device, stream))


def pairing_reserve(n, device=0):
    """Makes `device` ready for pairing batches of n items (self-test at its first use, the workspace): a later pairing_check_batch_device of up to n items only enqueues."""
    _check(_pairing_lib().bn254_pairing_reserve(n, device))


def dbg_pairing_batch(pairs, n_pairs, n=None, item_stride=None, device=-1, want_gt=True, form=None):
    """bn254_dbg_pairing_batch: (GT values or None, status bytes of the CHECK) from one run; device -1 is the host compile of the kernels' bodies, no GPU needed.
    form (1: the lane kernels, 2: the cooperative kernel; 0: as without it) forces the form of every launch through bn254_dbg_pairing_batch_form."""
    L = _pairing_lib()
    pairs, n, item_stride = _pairing_shape(pairs, n_pairs, n, item_stride)
    gt = (C.c_uint8 * max(384 * n, 1))() if want_gt else None
    status = (C.c_uint8 * max(n, 1))()
    if form is None:
        _check(L.bn254_dbg_pairing_batch(pairs, item_stride, n_pairs, n, gt, status, device))
    else:
        fn = L.bn254_dbg_pairing_batch_form
        fn.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _check(fn(pairs, item_stride, n_pairs, n, gt, status, device, form))
    return (bytes(gt)[:384 * n] if want_gt else None), bytes(status)[:n]


PAIRING_FORM_LANES, PAIRING_FORM_COOP = 1, 2

# ---- pairing batches with shared, prepared G2 points (bn254_g2_prepare, bn254_pairing_check_batch_shared) ----
G2_PREPARED_LEN = 19168
PAIRING_G1_LEN = 64


def g2_prepare(g2):
    """(status, record): the prepared record (G2_PREPARED_LEN bytes: header, affine point, 88 lines) of the G2 point x.c1 | x.c0 | y.c1 | y.c0 (128 bytes; all zero:
    the identity) when status is ACCEPT, else None with ERR_NOT_MEMBER / ERR_NOT_ON_CURVE / ERR_NOT_IN_SUBGROUP  (bn254_g2_prepare; host work, no device)."""
    g2 = bytes(g2)
    if len(g2) != 128:
        raise Bn254Error("g2_prepare: 128 bytes expected")
    fn = lib().bn254_g2_prepare
    fn.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    out = (C.c_uint8 * G2_PREPARED_LEN)(); st = C.c_uint8(0xEE)
    _check(fn(g2, out, C.byref(st)))
    return st.value, (bytes(out) if st.value == ACCEPT else None)


def pairing_packed_len(n_pairs, shared_mask):
    """bytes of a packed item: PAIRING_G1_LEN per shared position, PAIRING_PAIR_LEN per variable one"""
    return sum(PAIRING_G1_LEN if (shared_mask >> j) & 1 else PAIRING_PAIR_LEN for j in range(n_pairs))


def _shared_lib():
    L = lib()
    host = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_char_p, C.c_size_t]
    L.bn254_pairing_check_batch_shared.argtypes = host + [C.c_void_p, C.c_int]
    L.bn254_pairing_batch_shared.argtypes = host + [C.c_void_p, C.c_void_p, C.c_int]
    L.bn254_dbg_pairing_batch_shared.argtypes = host + [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bn254_pairing_check_batch_shared_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.bn254_pairing_check_batch_flags.argtypes = host + [C.c_void_p, C.c_int, C.c_uint]
    L.bn254_pairing_check_batch_flags_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    L.bn254_dbg_pairing_batch_rlc.argtypes = host + [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return L


def _shared_shape(items, n_pairs, shared_mask, prepared, n, item_stride):
    items = bytes(items)
    prepared = b"".join(prepared) if isinstance(prepared, (list, tuple)) else bytes(prepared)
    packed = pairing_packed_len(n_pairs, shared_mask)
    if item_stride is None:
        item_stride = packed
    if n is None:
        n = len(items) // item_stride if item_stride else 0
    if n and len(items) < (n - 1) * item_stride + packed:
        raise Bn254Error("pairing batch: the buffer is shorter than n packed items")
    if len(prepared) < G2_PREPARED_LEN * bin(shared_mask).count("1"):
        raise Bn254Error("pairing batch: fewer prepared records than shared positions")
    return items, prepared, n, item_stride


def pairing_check_batch_shared(items, n_pairs, shared_mask, prepared, n=None, item_stride=None, device=0, flags=0):
    """pairing_check_batch for items whose G2 point of every position j with bit j of shared_mask set is shared by the whole batch: `prepared` holds their records
    (g2_prepare; bytes, or a list of records) in ascending position order, and the items are PACKED -- 64 bytes (G1) per shared position, 192 per variable one.
    The status bytes are those of pairing_check_batch on the expanded items  (bn254_pairing_check_batch_shared).  flags: FLAG_RLC takes the call through
    bn254_pairing_check_batch_flags (the joint check of 64 items at a time from pairing_rlc_params() items per launch on, for shapes without a variable position -- others take the exact path; shared_mask 0 with no records is the
    all-variable item)."""
    L = _shared_lib()
    items, prepared, n, item_stride = _shared_shape(items, n_pairs, shared_mask, prepared, n, item_stride)
    status = (C.c_uint8 * max(n, 1))()
    if flags:
        _check(L.bn254_pairing_check_batch_flags(items, item_stride, n_pairs, shared_mask, prepared if shared_mask else None, n, status, device, flags))
    else:
        _check(L.bn254_pairing_check_batch_shared(items, item_stride, n_pairs, shared_mask, prepared, n, status, device))
    return bytes(status)[:n]


def pairing_batch_shared(items, n_pairs, shared_mask, prepared, n=None, item_stride=None, device=0):
    """(GT values, status bytes) as pairing_batch, for packed items with shared positions  (bn254_pairing_batch_shared)."""
    L = _shared_lib()
    items, prepared, n, item_stride = _shared_shape(items, n_pairs, shared_mask, prepared, n, item_stride)
    gt = (C.c_uint8 * max(384 * n, 1))(); status = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_pairing_batch_shared(items, item_stride, n_pairs, shared_mask, prepared, n, gt, status, device))
    return bytes(gt)[:384 * n], bytes(status)[:n]


def pairing_check_batch_shared_device(d_items, n_pairs, shared_mask, d_prepared, n, d_status, item_stride=None, device=0, stream=0, flags=0):
    """bn254_pairing_check_batch_shared_device on device pointers (ints; d_prepared 4-byte aligned): enqueues on `stream` and returns.  flags: FLAG_RLC takes the call
    through bn254_pairing_check_batch_flags_device, which synchronises `stream` once per launch that honours the flag."""
    L = _shared_lib()
    stride = pairing_packed_len(n_pairs, shared_mask) if item_stride is None else item_stride
    if flags:
        _check(L.bn254_pairing_check_batch_flags_device(d_items, stride, n_pairs, shared_mask, d_prepared, n, d_status, device, stream, flags))
    else:
        _check(L.bn254_pairing_check_batch_shared_device(d_items, stride, n_pairs, shared_mask, d_prepared, n, d_status, device, stream))


def set_pairing_rlc_params(rlc_min=-1):
    """bn254_set_pairing_rlc_params: FLAG_RLC on the pairing batch is honoured from rlc_min items per launch on (never below 64; negative: unchanged)."""
    fn = lib().bn254_set_pairing_rlc_params
    fn.argtypes = [C.c_long]; fn.restype = None
    fn(rlc_min)


def pairing_rlc_params():
    """rlc_min as it is now (bn254_pairing_rlc_params)."""
    fn = lib().bn254_pairing_rlc_params
    fn.argtypes = [C.POINTER(C.c_long)]
    out = (C.c_long * 1)()
    _check(fn(out))
    return int(out[0])


def pairing_rlc_state():
    """(launches that ran the joint check, groups they checked, groups that failed, launches on the exact path)  (bn254_pairing_rlc_state)."""
    fn = lib().bn254_pairing_rlc_state
    fn.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    _check(fn(out))
    return tuple(int(x) for x in out)


def dbg_set_pairing_rlc_max_var(max_var=-1):
    """bn254_dbg_set_pairing_rlc_max_var (tests): FLAG_RLC on the pairing batch is honoured for shapes of at most max_var variable positions (negative: the default,
    0); returns the value it replaces."""
    fn = lib().bn254_dbg_set_pairing_rlc_max_var
    fn.argtypes = [C.c_int]; fn.restype = C.c_int
    return fn(max_var)


def dbg_pairing_batch_rlc(items, n_pairs, shared_mask, prepared, n=None, item_stride=None, weights=None, device=-1, form=0):
    """bn254_dbg_pairing_batch_rlc: one weighted launch whatever the knob says.  weights: None (the real draw on a device, all 1 in the host compile) or n x 16 bytes
    big-endian, forced odd.  {"item_gt": n x 384 bytes (the final-exponentiated value of an item that reached the groups, on its weighted points; zero otherwise),
    "group_gt": groups x 384, "group_status": groups bytes, "status": n bytes}.  device -1 is the host compile."""
    L = _shared_lib()
    items, prepared, n, item_stride = _shared_shape(items, n_pairs, shared_mask, prepared, n, item_stride)
    if weights is not None:
        weights = bytes(weights)
        if len(weights) < 16 * n:
            raise Bn254Error("pairing batch: fewer weights than items")
    groups = (n + 63) // 64
    item_gt = (C.c_uint8 * max(384 * n, 1))(); grp_gt = (C.c_uint8 * max(384 * groups, 1))(); grp_st = (C.c_uint8 * max(groups, 1))(); status = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_dbg_pairing_batch_rlc(items, item_stride, n_pairs, shared_mask, prepared if shared_mask else None, n, weights, item_gt, grp_gt, grp_st, status, device, form))
    return {"item_gt": bytes(item_gt)[:384 * n], "group_gt": bytes(grp_gt)[:384 * groups], "group_status": bytes(grp_st)[:groups], "status": bytes(status)[:n]}


def dbg_pairing_batch_shared(items, n_pairs, shared_mask, prepared, n=None, item_stride=None, device=-1, want_gt=True, form=0):
    """bn254_dbg_pairing_batch_shared: (GT values or None, status bytes of the CHECK) from one run; device -1 is the host compile of the shared loader and the mixed
    Miller run; on a device form 1 forces the lane kernels, 2 the cooperative kernel."""
    L = _shared_lib()
    items, prepared, n, item_stride = _shared_shape(items, n_pairs, shared_mask, prepared, n, item_stride)
    gt = (C.c_uint8 * max(384 * n, 1))() if want_gt else None
    status = (C.c_uint8 * max(n, 1))()
    _check(L.bn254_dbg_pairing_batch_shared(items, item_stride, n_pairs, shared_mask, prepared, n, gt, status, device, form))
    return (bytes(gt)[:384 * n] if want_gt else None), bytes(status)[:n]


def set_pairing_params(coop_max=-1):
    """bn254_set_pairing_params: launches of up to coop_max items of a pairing batch take the cooperative twelve-lane form (0: always the lane form; clamped to the
    cooperative kernels' range; negative: unchanged)."""
    fn = lib().bn254_set_pairing_params
    fn.argtypes = [C.c_long]; fn.restype = None
    fn(coop_max)


def pairing_params():
    """coop_max as it is now (bn254_pairing_params)."""
    fn = lib().bn254_pairing_params
    fn.argtypes = [C.POINTER(C.c_long)]
    out = (C.c_long * 1)()
    _check(fn(out))
    return int(out[0])


def pairing_state():
    """(launches enqueued so far in the cooperative form, in the lane form)  (bn254_pairing_state)."""
    fn = lib().bn254_pairing_state
    fn.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    _check(fn(out))
    return int(out[0]), int(out[1])


def dbg_pairing_form(n_pairs, n):
    """The form a launch of n items of n_pairs pairs takes under the knobs as they are now: 1 lane, 2 cooperative (bn254_dbg_pairing_form, host only)."""
    fn = lib().bn254_dbg_pairing_form
    fn.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]
    out = C.c_int()
    _check(fn(n_pairs, n, C.byref(out)))
    return out.value


def dbg_pairing_plan(n_pairs, n):
    """{"ws_items", "pass_items", "passes", "pinned_bytes"} of a pairing batch of n items (bn254_dbg_pairing_plan, host only)."""
    out = (C.c_uint64 * 4)()
    _check(_pairing_lib().bn254_dbg_pairing_plan(n_pairs, n, out))
    return {"ws_items": out[0], "pass_items": out[1], "passes": out[2], "pinned_bytes": out[3]}


# ---- batch verification of KZG openings (bn254_kzg_key_prepare, bn254_kzg_verify_batch, include/bn254_verify.h) ----
KZG_OPENING_LEN = 192
KZG_KEY_LEN = 38424


def kzg_key_prepare(g1, g2, tau_g2):
    """(status, key): the KZG key (KZG_KEY_LEN bytes of plain data: header, g1, the prepared records of g2 and tau_g2) when status is ACCEPT, else None with the first
    failure over g1 (64 bytes), g2, tau_g2 (128 bytes each)  (bn254_kzg_key_prepare; host work, no device)."""
    g1, g2, tau_g2 = bytes(g1), bytes(g2), bytes(tau_g2)
    if len(g1) != 64 or len(g2) != 128 or len(tau_g2) != 128:
        raise Bn254Error("kzg_key_prepare: 64, 128 and 128 bytes expected")
    fn = lib().bn254_kzg_key_prepare
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    out = (C.c_uint8 * KZG_KEY_LEN)(); st = C.c_uint8(0xEE)
    _check(fn(g1, g2, tau_g2, out, C.byref(st)))
    return st.value, (bytes(out) if st.value == ACCEPT else None)


def _kzg_shape(key, openings, n, stride):
    key, openings = bytes(key), bytes(openings)
    if stride is None:
        stride = KZG_OPENING_LEN
    if n is None:
        n = len(openings) // stride if stride else 0
    if len(key) < KZG_KEY_LEN:
        raise Bn254Error("KZG batch: the key is shorter than KZG_KEY_LEN")
    if n and stride >= KZG_OPENING_LEN and len(openings) < (n - 1) * stride + KZG_OPENING_LEN:
        raise Bn254Error("KZG batch: the buffer is shorter than n openings")
    return key, openings, n, stride


def kzg_verify_batch(key, openings, n=None, stride=None, device=0, flags=0):
    """n status bytes: ACCEPT where e(C - y g1 + z H, g2) e(-H, tau_g2) == 1 for the opening C | H | z | y (KZG_OPENING_LEN bytes), REJECT where it is not, or the
    loader error.  flags: FLAG_STRICT_SCALARS, FLAG_RLC (the joint check over groups of 64 openings, honoured from kzg_params() openings on)  (bn254_kzg_verify_batch)."""
    fn = lib().bn254_kzg_verify_batch
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    key, openings, n, stride = _kzg_shape(key, openings, n, stride)
    status = (C.c_uint8 * max(n, 1))()
    _check(fn(key, openings, stride, n, status, device, flags))
    return bytes(status)[:n]


def kzg_verify_batch_device(d_key, d_openings, n, d_status, stride=KZG_OPENING_LEN, device=0, stream=0, flags=0):
    """bn254_kzg_verify_batch_device on device pointers (ints; d_key 4-byte aligned): enqueues on `stream` and returns (with FLAG_RLC honoured it synchronises once)."""
    fn = lib().bn254_kzg_verify_batch_device
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    _check(fn(d_key, d_openings, stride, n, d_status, device, stream, flags))


def kzg_reserve(n, device=0):
    """Makes `device` ready for KZG batches of n openings: a later kzg_verify_batch_device of up to n openings without FLAG_RLC only enqueues  (bn254_kzg_reserve)."""
    fn = lib().bn254_kzg_reserve
    fn.argtypes = [C.c_size_t, C.c_int]
    _check(fn(n, device))


def set_kzg_params(rlc_min=-1):
    """bn254_set_kzg_params: FLAG_RLC is honoured from rlc_min openings per launch on (never below 64; negative: unchanged)."""
    fn = lib().bn254_set_kzg_params
    fn.argtypes = [C.c_long]; fn.restype = None
    fn(rlc_min)


def kzg_params():
    """rlc_min as it is now (bn254_kzg_params)."""
    fn = lib().bn254_kzg_params
    fn.argtypes = [C.POINTER(C.c_long)]
    out = (C.c_long * 1)()
    _check(fn(out))
    return int(out[0])


def kzg_state():
    """(launches that ran the joint check, groups they checked, groups that failed, launches on the exact path)  (bn254_kzg_state)."""
    fn = lib().bn254_kzg_state
    fn.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    _check(fn(out))
    return tuple(int(x) for x in out)


def dbg_kzg_fold(key, openings, n=None, stride=None, weights=None, flags=0, device=-1, form=0, want_groups=False):
    """bn254_dbg_kzg_fold: {"f", "h": n x 64 bytes (vp_p(0), vp_p(1); zero: identity or decided), "inf": n x 2 flags, "status": n bytes, "groups": None or a list of
    (F sum, H sum, flags, status) per 64 openings}.  weights: None or n 128-bit integers (FLAG_RLC; forced odd); device -1 is the host compile, no GPU needed."""
    fn = lib().bn254_dbg_kzg_fold
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    key, openings, n, stride = _kzg_shape(key, openings, n, stride)
    wb = None if weights is None else b"".join(int(w).to_bytes(16, "big") for w in weights)
    if wb is not None and len(wb) != 16 * n:
        raise Bn254Error("dbg_kzg_fold: one weight per opening")
    groups = (n + 63) // 64
    f = (C.c_uint8 * max(64 * n, 1))(); h = (C.c_uint8 * max(64 * n, 1))(); inf = (C.c_uint8 * max(2 * n, 1))(); status = (C.c_uint8 * max(n, 1))()
    grp = (C.c_uint8 * max(131 * groups, 1))() if want_groups else None
    _check(fn(key, openings, stride, n, wb, flags, f, h, inf, status, grp, device, form))
    out = {"f": bytes(f)[:64 * n], "h": bytes(h)[:64 * n], "inf": bytes(inf)[:2 * n], "status": bytes(status)[:n], "groups": None}
    if want_groups:
        g = bytes(grp)
        out["groups"] = [(g[131 * q:131 * q + 64], g[131 * q + 64:131 * q + 128], g[131 * q + 128:131 * q + 130], g[131 * q + 130]) for q in range(groups)]
    return out


# ---- batch verification of KZG batch-opening proofs (bn254_kzg_verify_folded_batch, include/bn254_verify.h) ----
KZG_FOLD_MAX_DIGESTS = 13
KZG_FOLD_MAX_DATA = 64


def kzg_fold_len(n_digests, data_len=0):
    """BN254_KZG_FOLD_LEN: D_0 .. D_{k-1} (64 each) | H (64) | z (32) | y_0 .. y_{k-1} (32 each) | data"""
    return 96 + 96 * n_digests + data_len


def _kzg_fold_shape(key, records, n, stride, n_digests, data_len):
    key, records = bytes(key), bytes(records)
    rec = kzg_fold_len(n_digests, data_len)
    if stride is None:
        stride = rec
    if n is None:
        n = len(records) // stride if stride else 0
    if len(key) < KZG_KEY_LEN:
        raise Bn254Error("KZG batch: the key is shorter than KZG_KEY_LEN")
    if n and 1 <= n_digests <= KZG_FOLD_MAX_DIGESTS and 0 <= data_len <= KZG_FOLD_MAX_DATA and stride >= rec and len(records) < (n - 1) * stride + rec:
        raise Bn254Error("KZG batch: the buffer is shorter than n records")
    return key, records, n, stride


def kzg_verify_folded_batch(key, records, n_digests, data_len=0, n=None, stride=None, device=0, flags=0):
    """n status bytes for batch-opening records of n_digests digests and data_len bytes of caller data each (kzg_fold_len bytes): gamma from the SHA-256 transcript over
    the point, the digests, the claimed values and the data; ACCEPT where e(sum gamma^i D_i - (sum gamma^i y_i) g1 + z H, g2) e(-H, tau_g2) == 1, REJECT where it is
    not, or the loader error.  flags as kzg_verify_batch  (bn254_kzg_verify_folded_batch)."""
    fn = lib().bn254_kzg_verify_folded_batch
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    key, records, n, stride = _kzg_fold_shape(key, records, n, stride, n_digests, data_len)
    status = (C.c_uint8 * max(n, 1))()
    _check(fn(key, records, stride, n, n_digests, data_len, status, device, flags))
    return bytes(status)[:n]


def kzg_verify_folded_batch_device(d_key, d_records, n, n_digests, d_status, data_len=0, stride=None, device=0, stream=0, flags=0):
    """bn254_kzg_verify_folded_batch_device on device pointers (ints; d_key 4-byte aligned): enqueues on `stream` and returns (with FLAG_RLC honoured it synchronises once)."""
    fn = lib().bn254_kzg_verify_folded_batch_device
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    _check(fn(d_key, d_records, kzg_fold_len(n_digests, data_len) if stride is None else stride, n, n_digests, data_len, d_status, device, stream, flags))


def kzg_fold_reserve(n, n_digests, device=0):
    """Makes `device` ready for batches of n records of n_digests digests: a later kzg_verify_folded_batch_device of up to n such records without FLAG_RLC only
    enqueues  (bn254_kzg_fold_reserve)."""
    fn = lib().bn254_kzg_fold_reserve
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_int]
    _check(fn(n, n_digests, device))


def dbg_kzg_fold_proof(key, records, n_digests, data_len=0, n=None, stride=None, weights=None, flags=0, device=-1, form=0, want_groups=False):
    """bn254_dbg_kzg_fold_proof: what dbg_kzg_fold returns, and "gamma" (n x 32 bytes: the digest gamma is reduced from) and "yhat" (n x 32 bytes, canonical); both zero
    for a record the loader decided.  device -1 is the host compile, no GPU needed."""
    fn = lib().bn254_dbg_kzg_fold_proof
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int, C.c_int]
    key, records, n, stride = _kzg_fold_shape(key, records, n, stride, n_digests, data_len)
    wb = None if weights is None else b"".join(int(w).to_bytes(16, "big") for w in weights)
    if wb is not None and len(wb) != 16 * n:
        raise Bn254Error("dbg_kzg_fold_proof: one weight per record")
    groups = (n + 63) // 64
    fold = (C.c_uint8 * max(64 * n, 1))()
    f = (C.c_uint8 * max(64 * n, 1))(); h = (C.c_uint8 * max(64 * n, 1))(); inf = (C.c_uint8 * max(2 * n, 1))(); status = (C.c_uint8 * max(n, 1))()
    grp = (C.c_uint8 * max(131 * groups, 1))() if want_groups else None
    _check(fn(key, records, stride, n, n_digests, data_len, wb, flags, fold, f, h, inf, status, grp, device, form))
    fb = bytes(fold)
    out = {"gamma": b"".join(fb[64 * i:64 * i + 32] for i in range(n)), "yhat": b"".join(fb[64 * i + 32:64 * i + 64] for i in range(n)),
           "f": bytes(f)[:64 * n], "h": bytes(h)[:64 * n], "inf": bytes(inf)[:2 * n], "status": bytes(status)[:n], "groups": None}
    if want_groups:
        g = bytes(grp)
        out["groups"] = [(g[131 * q:131 * q + 64], g[131 * q + 64:131 * q + 128], g[131 * q + 128:131 * q + 130], g[131 * q + 130]) for q in range(groups)]
    return out


def dbg_kzg_fold_plan(n_digests, weighted, n, lane_budget=0, joint_g=-1):
    """rows of the G1 walk of n records of n_digests digests, or None when the shape does not plan  (bn254_dbg_kzg_fold_plan; host only)."""
    fn = lib().bn254_dbg_kzg_fold_plan
    fn.argtypes = [C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    rows = C.c_int(0)
    return int(rows.value) if fn(n_digests, 1 if weighted else 0, n, lane_budget, joint_g, C.byref(rows)) == 0 else None


# ---- batch G1 multi-scalar multiplication with per-item and shared bases (bn254_g1_bases_prepare, bn254_g1_msm_batch, include/bn254_verify.h) ----
G1_MSM_MAX_VAR = 16
G1_MSM_MAX_UNIT = 4
G1_MSM_MAX_SHARED = 16


def g1_msm_item_len(n_var, n_unit, n_shared):
    """BN254_G1_MSM_ITEM_LEN: n_var pairs (point 64, scalar 32), n_unit points (64), n_shared scalars (32)."""
    return 96 * n_var + 64 * n_unit + 32 * n_shared


class G1Bases:
    """Owner of a bn254_g1_bases_prepare handle: the window tables of up to G1_MSM_MAX_SHARED points on one device.  close() (or the end of a `with`) frees them after
    waiting for the device."""

    def __init__(self, handle, device):
        self._h, self.device = handle, device

    @property
    def handle(self):
        if not self._h:
            raise Bn254Error("G1Bases: the handle has been freed")
        return self._h

    def __len__(self):
        fn = lib().bn254_g1_bases_count
        fn.argtypes = [C.c_void_p]; fn.restype = C.c_size_t
        return int(fn(self.handle))

    def close(self):
        if self._h:
            fn = lib().bn254_g1_bases_free
            fn.argtypes = [C.c_void_p]; fn.restype = None
            fn(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g1_bases_prepare(points, device=0):
    """(status, G1Bases or None): the shared bases of g1_msm_batch from 1 .. G1_MSM_MAX_SHARED points of 64 bytes; status is ACCEPT, or the first failure (a coordinate
    >= p: ERR_NOT_MEMBER, off the curve: ERR_NOT_ON_CURVE) and no handle  (bn254_g1_bases_prepare)."""
    points = bytes(points)
    if len(points) % 64:
        raise Bn254Error("g1_bases_prepare: points of 64 bytes expected")
    fn = lib().bn254_g1_bases_prepare
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    h = C.c_void_p(None); st = C.c_uint8(0xEE)
    _check(fn(points, len(points) // 64, device, C.byref(h), C.byref(st)))
    return st.value, (G1Bases(h.value, device) if st.value == ACCEPT and h.value else None)


def _g1_msm_shape(items, n_var, n_unit, n_shared, n, stride):
    items = bytes(items)
    ilen = g1_msm_item_len(n_var, n_unit, n_shared)
    if stride is None:
        stride = ilen
    if n is None:
        n = len(items) // stride if stride else 0
    if n and stride >= ilen and len(items) < (n - 1) * stride + ilen:
        raise Bn254Error("G1 MSM batch: the buffer is shorter than n items")
    return items, n, stride


def g1_msm_batch(items, n_var, n_unit, n_shared, bases=None, n=None, stride=None, device=0, flags=0):
    """(out, status): per item the 64 bytes x | y of  sum k_t P_t + sum U_t + sum c_j B_j  (zero: the identity, or an item that ended in an error) and its status byte
    (ACCEPT, or the loader error).  bases: a G1Bases (n_shared > 0).  flags: FLAG_STRICT_SCALARS  (bn254_g1_msm_batch)."""
    fn = lib().bn254_g1_msm_batch
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
    items, n, stride = _g1_msm_shape(items, n_var, n_unit, n_shared, n, stride)
    out = (C.c_uint8 * max(64 * n, 1))(); status = (C.c_uint8 * max(n, 1))()
    _check(fn(items, stride, n_var, n_unit, n_shared, bases.handle if bases is not None else None, n, out, status, device, flags))
    return bytes(out)[:64 * n], bytes(status)[:n]


def g1_msm_batch_device(d_items, n_var, n_unit, n_shared, n, d_out, d_status, bases=None, stride=None, device=0, stream=0, flags=0):
    """bn254_g1_msm_batch_device on device pointers (ints): enqueues on `stream` and returns; d_out receives 64 n bytes, d_status n."""
    fn = lib().bn254_g1_msm_batch_device
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    _check(fn(d_items, g1_msm_item_len(n_var, n_unit, n_shared) if stride is None else stride, n_var, n_unit, n_shared, bases.handle if bases is not None else None, n, d_out,
              d_status, device, stream, flags))


def g1_msm_reserve(n, n_var, n_unit, n_shared, device=0):
    """Makes `device` ready for batches of n items of this shape: a later g1_msm_batch_device of up to n such items only enqueues  (bn254_g1_msm_reserve)."""
    fn = lib().bn254_g1_msm_reserve
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    _check(fn(n, n_var, n_unit, n_shared, device))


def dbg_g1_msm_batch(items, n_var, n_unit, n_shared, base_points=b"", n=None, stride=None, flags=0, lane_budget=0, joint_g=-1, device=-1):
    """bn254_dbg_g1_msm_batch, one pass with the plan's form forced: {"out": n x 64 bytes, "status": n bytes, "rows", "var_rows", "form": "split" | "unsplit" | "joint",
    "chain"}.  base_points: the shared bases as raw 64-byte points.  device -1 is the host compile, no GPU needed."""
    fn = lib().bn254_dbg_g1_msm_batch
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                   C.POINTER(C.c_int), C.c_int]
    items, n, stride = _g1_msm_shape(items, n_var, n_unit, n_shared, n, stride)
    base_points = bytes(base_points)
    out = (C.c_uint8 * max(64 * n, 1))(); status = (C.c_uint8 * max(n, 1))(); info = (C.c_int * 6)()
    _check(fn(items, stride, n_var, n_unit, n_shared, base_points or None, len(base_points) // 64, n, flags, lane_budget, joint_g, out, status, info, device))
    return {"out": bytes(out)[:64 * n], "status": bytes(status)[:n], "rows": info[0], "var_rows": info[1], "form": ("split", "unsplit", "joint")[info[4]], "chain": info[5]}


def dbg_g1_msm_batch_plan(n_var, n_unit, n_shared, n, lane_budget=0, joint_g=-1):
    """rows of the G1 walk of n items of a shape, or None when the shape does not plan  (bn254_dbg_g1_msm_batch_plan; host only)."""
    fn = lib().bn254_dbg_g1_msm_batch_plan
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    rows = C.c_int(0)
    return int(rows.value) if fn(n_var, n_unit, n_shared, n, lane_budget, joint_g, C.byref(rows)) == 0 else None


def dbg_g1_msm_batch_state(n_var, n_unit, n_shared):
    """{"pass_items": items of a pass of the shape (BN254_G1_MSM_PASS applied), "formula_items", "bytes_per_item", "allocs": device and pinned allocations the entry has
    made so far}  (bn254_dbg_g1_msm_batch_state; host only)."""
    fn = lib().bn254_dbg_g1_msm_batch_state
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    _check(fn(n_var, n_unit, n_shared, out))
    return {"pass_items": int(out[0]), "formula_items": int(out[1]), "bytes_per_item": int(out[2]), "allocs": int(out[3])}


G16_LOADER_LANES, G16_LOADER_COMPACT, G16_LOADER_WIDE, G16_LOADER_WIDE8 = range(4)      # form of dbg_g16_loader
G16_LOADER_POINTS_LEN = 320                                                              # A (64) | B (128) | C (64) | L (64)


def _loader_args():
    return [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.POINTER(C.c_int), C.c_int]


def dbg_g16_loader(key, proofs, public_inputs, n_public, n, form, flags=0, misalign=0, proof_stride=256, device=0):
    """The loader stage of a Groth16 batch under one prepared key, in a forced form (bn254_dbg_g16_loader): {"status": n bytes as the stage leaves them, "points": n
    records A | B | C | L of 320 bytes (per slot when form is G16_LOADER_COMPACT), "slot_status" / "slot_proof" (compaction only), "form", "chunks", "reduce": None |
    "k_g16_msm_reduce" | "k_g16_msm_reduce8", "tables": "comb" | "bytes" | "fw13" (the sum's kernel), "check_scalars", "comb_digits"} -- the last six as the launcher
    recorded them at its launch sites."""
    fn = lib().bn254_dbg_g16_loader
    fn.argtypes = _loader_args()
    st = (C.c_uint8 * n)(); sst = (C.c_uint8 * n)(); sp = (C.c_uint32 * n)(); pts = (C.c_uint8 * (G16_LOADER_POINTS_LEN * n))(); info = (C.c_int * 6)()
    compact = form == G16_LOADER_COMPACT
    _check(fn(key.handle, bytes(proofs), proof_stride, bytes(public_inputs) or None, n_public, n, flags, form, misalign, st, sst if compact else None, sp if compact else None, pts,
              info, device))
    pts = bytes(pts)
    return {"status": bytes(st), "points": [pts[G16_LOADER_POINTS_LEN * i:G16_LOADER_POINTS_LEN * (i + 1)] for i in range(n)],
            "slot_status": bytes(sst) if compact else None, "slot_proof": list(sp) if compact else None, "form": info[0], "chunks": info[1],
            "reduce": (None, "k_g16_msm_reduce", "k_g16_msm_reduce8")[info[2]], "tables": ("fw13", "comb", "bytes")[info[3]], "check_scalars": bool(info[4]),
            "comb_digits": bool(info[5])}


def dbg_g16_loader_keys(key_set, key_index, proofs, public_inputs, n=None, flags=0, misalign=0, proof_stride=256, input_stride=None, device=0):
    """The loader stage of a batch over a KeySet in its grouped form (bn254_dbg_g16_loader_keys): {"n_slots", "slot_proof": per slot the proof index or None for a
    padding slot, "slot_status": bytes, "points": per slot A | B | C | L}."""
    fn = lib().bn254_dbg_g16_loader_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.POINTER(C.c_size_t), C.c_int]
    idx = key_set._index(key_index)
    n = len(idx) if n is None else n
    counts = {}
    for k in idx:
        counts[k] = counts.get(k, 0) + 1
    slots = sum((c + 63) // 64 * 64 for c in counts.values())
    sp = (C.c_uint32 * max(slots, 1))(); sst = (C.c_uint8 * max(slots, 1))(); pts = (C.c_uint8 * max(G16_LOADER_POINTS_LEN * slots, 1))(); ns = C.c_size_t(0)
    _check(fn(key_set._arr, len(key_set.keys), idx.buffer_info()[0] if len(idx) else None, bytes(proofs), proof_stride, bytes(public_inputs) or None,
              key_set.input_stride if input_stride is None else input_stride, n, flags, misalign, slots, sp, sst, pts, C.byref(ns), device))
    pts = bytes(pts)
    return {"n_slots": int(ns.value), "slot_proof": [None if v == 0xffffffff else int(v) for v in sp][:slots], "slot_status": bytes(sst)[:slots],
            "points": [pts[G16_LOADER_POINTS_LEN * i:G16_LOADER_POINTS_LEN * (i + 1)] for i in range(slots)]}
