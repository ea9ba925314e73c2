//! The reference's surface (`verifier/src/lib.rs:29-75`) over the MI355X library, plus `verify_batch`.
//!
//! * `Groth16Verifier::verify(proof, vk, public_inputs)` -> `Result<bool, Groth16Error>`: `Ok(true)` / `Ok(false)` / `Err(PrepareInputsFailed)`
//!   (`groth16/verify.rs:54-56,77`); everything the reference turns into a panic through `unwrap` (`lib.rs:45-46`) panics here too.
//! * `PlonkVerifier::verify` -> `Result<bool, PlonkError>`: never `Ok(false)` (`plonk/verify.rs:316`).
//! * `verify_batch`: one status per proof, nothing panics; `PreparedGroth16Vk` / `PreparedPlonkVk` keep the key work that the reference repeats on every call.
//! Public inputs are 32-byte big-endian values used modulo r, as `bn::Fr::from_slice` + `AffineG1 * Fr` use them.
//! NOT COMPILED in the repository's build image (no Rust toolchain there): see ../README.md.
use bn254_verify_amd_sys as sys;
use core::ffi::{c_int, c_void, CStr};

/// `groth16/error.rs:4-15`: the one error `verify_groth16` returns.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Groth16Error { PrepareInputsFailed }
/// `plonk/error.rs`: the errors `verify_plonk` returns.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum PlonkError { InvalidWitness, OpeningPolyMismatch, PairingCheckFailed, Bsb22CommitmentMismatch, InverseNotFound }

/// Outcome of one proof of a batch: the reference's `Result`, with its panics as a value.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Status {
    Accept, Reject, NotMember, NotOnCurve, NotInSubgroup, InputLen, Malformed, OpeningMismatch, PairingFailed, Bsb22Mismatch, Inverse, Unknown(u8),
}
impl From<u8> for Status {
    fn from(s: u8) -> Self {
        match s {
            sys::BN254_ACCEPT => Status::Accept, sys::BN254_REJECT => Status::Reject, sys::BN254_ERR_NOT_MEMBER => Status::NotMember,
            sys::BN254_ERR_NOT_ON_CURVE => Status::NotOnCurve, sys::BN254_ERR_NOT_IN_SUBGROUP => Status::NotInSubgroup, sys::BN254_ERR_INPUT_LEN => Status::InputLen,
            sys::BN254_ERR_MALFORMED => Status::Malformed, sys::BN254_ERR_OPENING_MISMATCH => Status::OpeningMismatch, sys::BN254_ERR_PAIRING_FAILED => Status::PairingFailed,
            sys::BN254_ERR_BSB22_MISMATCH => Status::Bsb22Mismatch, sys::BN254_ERR_INVERSE => Status::Inverse, x => Status::Unknown(x),
        }
    }
}
/// What keeps the library from running: not an outcome of a proof.  `message` is `bn254_last_error()` of the call.
#[derive(Debug, Clone)]
pub enum Error {
    /// no device, HIP error, bad argument, out of memory: `code` is the `BN254_E_*` value
    Infrastructure { code: c_int, message: String },
    /// `BN254_E_SELFTEST`: a shipped kernel disagrees with its known answer on the device, which is refused until a `device_selftest` on it passes; the
    /// message names the first failing check
    SelfTest { message: String },
}
impl Error {
    pub fn code(&self) -> c_int { match self { Error::Infrastructure { code, .. } => *code, Error::SelfTest { .. } => sys::BN254_E_SELFTEST } }
    pub fn message(&self) -> &str { match self { Error::Infrastructure { message, .. } | Error::SelfTest { message } => message } }
}
fn check(rc: c_int) -> Result<(), Error> {
    if rc == sys::BN254_OK { return Ok(()); }
    let message = unsafe { CStr::from_ptr(sys::bn254_last_error()) }.to_string_lossy().into_owned();
    Err(if rc == sys::BN254_E_SELFTEST { Error::SelfTest { message } } else { Error::Infrastructure { code: rc, message } })
}

/// What `device_selftest` found: the checks that disagree (bit k of `failed_mask` = check k, `failed` their names) and the wall time of the run.
#[derive(Debug, Clone)]
pub struct SelfTestReport { pub passed: bool, pub failed_mask: u32, pub failed: Vec<String>, pub ms: f32, pub message: Option<String> }

/// The known-answer self-test of the verdict kernels on `device`, now (`bn254_device_selftest`): an operator's health check.  The library runs it by itself before a
/// device is first used; this call runs it whatever ran before, and its result replaces the device's recorded state (a pass clears an earlier failure).  A check
/// that disagrees is a report with `passed == false`, not an `Err`: `Err` is for a run that could not be made.
pub fn device_selftest(device: i32) -> Result<SelfTestReport, Error> {
    let (mut mask, mut ms) = (0 as core::ffi::c_uint, 0f32);
    let rc = unsafe { sys::bn254_device_selftest(device as c_int, &mut mask, &mut ms) };
    let message = match check(rc) { Ok(()) => None, Err(Error::SelfTest { message }) => Some(message), Err(e) => return Err(e) };
    let failed = (0..sys::BN254_SELFTEST_NUM_CHECKS as c_int).filter(|k| mask >> k & 1 == 1)
        .map(|k| unsafe { CStr::from_ptr(sys::bn254_selftest_check_name(k)) }.to_string_lossy().into_owned()).collect();
    Ok(SelfTestReport { passed: rc == sys::BN254_OK, failed_mask: mask as u32, failed, ms, message })
}
/// (state, failed mask) of the device's recorded self-test: -1 not run yet, 0 failed, 1 passed, 2 skipped (`BN254_SELFTEST=0`).  Touches no device.
pub fn device_selftest_state(device: i32) -> Result<(i32, u32), Error> {
    let (mut state, mut mask) = (-1 as c_int, 0 as core::ffi::c_uint);
    check(unsafe { sys::bn254_device_selftest_state(device as c_int, &mut state, &mut mask) })?;
    Ok((state as i32, mask as u32))
}

/// Which reading of a compressed G2 point the key loader uses: the reference's literal function, or gnark's.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum VkMode { Reference = 0, Gnark = 1 }

pub const FLAG_STRICT_SCALARS: u32 = sys::BN254_FLAG_STRICT_SCALARS as u32;
pub const FLAG_RLC: u32 = sys::BN254_FLAG_RLC as u32;
/// Records are gnark's compressed proofs (A 32 | B 64 | C 32, `proof_stride >= 128`), decompressed on the device; see the header for the status of each record.
pub const FLAG_COMPRESSED_PROOFS: u32 = sys::BN254_FLAG_COMPRESSED_PROOFS as u32;

/// Smallest Groth16 record the flags allow: 128 bytes for compressed proofs, 256 for the raw layout.
fn g16_min_stride(flags: u32) -> usize { if flags & FLAG_COMPRESSED_PROOFS != 0 { 128 } else { 256 } }

fn flatten(proofs: &[&[u8]], min_stride: usize) -> (Vec<u8>, usize) {
    let stride = proofs.iter().map(|p| p.len()).max().unwrap_or(min_stride).max(min_stride);
    let mut buf = vec![0u8; stride * proofs.len()];
    for (i, p) in proofs.iter().enumerate() { buf[i * stride..i * stride + p.len()].copy_from_slice(p); }
    (buf, stride)
}

/// SP1's committed_values_digest of a proof's public values: SHA-256 with the top three bits of byte 0 cleared (the circuit's input 1; input 0 is the program's
/// vkey hash).
pub fn sp1_public_values_digest(public_values: &[u8]) -> Result<[u8; 32], Error> {
    let mut out = [0u8; 32];
    check(unsafe { sys::bn254_sp1_public_values_digest(public_values.as_ptr(), public_values.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// The host buffers of an SP1 batch: the values concatenated and the n + 1 offsets; the vkey hashes as one hash (stride 0) or one per proof (stride 32).
fn sp1_buffers(vkey_hashes: &[[u8; 32]], public_values: &[&[u8]]) -> (Vec<u8>, Vec<u64>, Vec<u8>, usize) {
    assert!(vkey_hashes.len() == 1 || vkey_hashes.len() == public_values.len(), "one vkey hash, or one per proof");
    let mut pv = Vec::new();
    let mut offs = Vec::with_capacity(public_values.len() + 1);
    for v in public_values { offs.push(pv.len() as u64); pv.extend_from_slice(v); }
    offs.push(pv.len() as u64);
    let vk: Vec<u8> = vkey_hashes.iter().flat_map(|h| h.iter().copied()).collect();
    let stride = if vkey_hashes.len() == 1 && public_values.len() != 1 { 0 } else { 32 };
    (pv, offs, vk, stride)
}

/// `load_groth16_verifying_key_from_bytes` + `pairing(alpha, beta)` (`groth16/converter.rs:28-89`, `groth16/verify.rs:70`), done once.
pub struct PreparedGroth16Vk { h: *mut sys::Bn254G16Pvk }
unsafe impl Send for PreparedGroth16Vk {}
unsafe impl Sync for PreparedGroth16Vk {}   // the handle is immutable; the library serialises batches per (key, device)
impl PreparedGroth16Vk {
    pub fn new(vk: &[u8], mode: VkMode) -> Result<Self, Error> {
        let mut h = core::ptr::null_mut();
        check(unsafe { sys::bn254_groth16_vk_prepare(vk.as_ptr(), vk.len(), mode as u32, &mut h) })?;
        Ok(Self { h })
    }
    /// Many keys prepared in one call, on `device` (`bn254_groth16_vk_prepare_batch`): entry `i` is `vks[i]` prepared -- equal to `new(vks[i], mode)` in everything a
    /// caller can observe -- or `None` for a key that does not load (where `new` answers `BN254_E_VK`).  The keys are independent: each is dropped on its own.
    pub fn prepare_batch(vks: &[&[u8]], mode: VkMode, device: i32) -> Result<Vec<Option<Self>>, Error> {
        static NONE: u8 = 0;
        let ptrs: Vec<*const u8> = vks.iter().map(|v| if v.is_empty() { &NONE as *const u8 } else { v.as_ptr() }).collect();
        let lens: Vec<usize> = vks.iter().map(|v| v.len()).collect();
        let mut out: Vec<*mut sys::Bn254G16Pvk> = vec![core::ptr::null_mut(); vks.len()];
        let mut status: Vec<c_int> = vec![0; vks.len()];
        check(unsafe { sys::bn254_groth16_vk_prepare_batch(ptrs.as_ptr() as *mut *const u8, lens.as_ptr(), vks.len(), mode as u32, device, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok(out.into_iter().map(|h| if h.is_null() { None } else { Some(Self { h }) }).collect())
    }
    pub fn num_public(&self) -> usize { unsafe { sys::bn254_groth16_vk_num_public(self.h) } }
    /// Allocations ahead of the first batch (otherwise the first call makes them).
    pub fn reserve(&self, n: usize, device: i32) -> Result<(), Error> { check(unsafe { sys::bn254_groth16_reserve(self.h, n, device) }) }
    /// `n` proofs, `proof_stride` bytes apart (>= 256: A | B | C as gnark writes them; with `FLAG_COMPRESSED_PROOFS` >= 128: gnark's compressed form), `n_public`
    /// 32-byte inputs each; host buffers in, status bytes out.
    pub fn verify_batch_raw(&self, proofs: &[u8], proof_stride: usize, public_inputs: &[u8], n_public: usize, n: usize, device: i32, flags: u32) -> Result<Vec<Status>, Error> {
        assert!(proof_stride >= g16_min_stride(flags) && proofs.len() >= n * proof_stride && public_inputs.len() >= n * n_public * 32);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_groth16_verify_batch(self.h, proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), n_public, n, st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// The same over the GPUs selected by `device_mask` (contiguous shards, one host thread per device: SURVEY.md section 8(e)).
    pub fn verify_batch_multi_raw(&self, proofs: &[u8], proof_stride: usize, public_inputs: &[u8], n_public: usize, n: usize, device_mask: u64, flags: u32) -> Result<Vec<Status>, Error> {
        assert!(proof_stride >= g16_min_stride(flags) && proofs.len() >= n * proof_stride && public_inputs.len() >= n * n_public * 32);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_groth16_verify_batch_multi(self.h, proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), n_public, n, st.as_mut_ptr(), device_mask, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// Proofs and inputs already in device memory; enqueues on `hip_stream` and returns (BN254_FLAG_RLC: after one stream synchronisation).
    /// # Safety
    /// The three device pointers must be valid for the sizes implied by `n`, `proof_stride`, `n_public` until the stream has run the batch.
    pub unsafe fn verify_batch_device(&self, d_proofs: *const c_void, proof_stride: usize, d_inputs: *const c_void, n_public: usize, n: usize, d_status: *mut c_void, device: i32,
                                      hip_stream: *mut c_void, flags: u32) -> Result<(), Error> {
        check(sys::bn254_groth16_verify_batch_device(self.h, d_proofs, proof_stride, d_inputs, n_public, n, d_status, device, hip_stream, flags))
    }
    /// SP1 proofs from their public values: `n = public_values.len()` proofs `proof_stride` bytes apart, each verified against vkey_hash_i | digest(values_i), the
    /// digest made on the device.  `vkey_hashes`: one for the whole batch or one per proof.  `flags` as `verify_batch_raw` (a key of another width than 2 gives
    /// `Status::InputLen`).
    pub fn verify_sp1_batch(&self, proofs: &[u8], proof_stride: usize, vkey_hashes: &[[u8; 32]], public_values: &[&[u8]], device: i32, flags: u32) -> Result<Vec<Status>, Error> {
        let n = public_values.len();
        assert!(proof_stride >= g16_min_stride(flags) && proofs.len() >= n * proof_stride);
        let (pv, offs, vk, stride) = sp1_buffers(vkey_hashes, public_values);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_sp1_groth16_verify_batch(self.h, proofs.as_ptr(), proof_stride, vk.as_ptr(), stride, pv.as_ptr(), offs.as_ptr(), n, st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
}
impl Drop for PreparedGroth16Vk { fn drop(&mut self) { unsafe { sys::bn254_groth16_vk_free(self.h) } } }

pub struct Groth16Verifier;
impl Groth16Verifier {
    /// `Groth16Verifier::verify` (`lib.rs:44-49`).  Panics where the reference panics (loader errors through `unwrap`, short buffers, flag `0b00`).
    pub fn verify(proof: &[u8], vk: &[u8], public_inputs: &[[u8; 32]]) -> Result<bool, Groth16Error> {
        let inputs: Vec<u8> = public_inputs.iter().flatten().copied().collect();
        let mut st = 0u8;
        let rc = unsafe { sys::bn254_groth16_verify(proof.as_ptr(), proof.len(), vk.as_ptr(), vk.len(), inputs.as_ptr(), public_inputs.len(), sys::BN254_VK_REFERENCE, &mut st) };
        check(rc).expect("bn254 infrastructure error");
        match Status::from(st) {
            Status::Accept => Ok(true),
            Status::Reject => Ok(false),
            Status::InputLen => Err(Groth16Error::PrepareInputsFailed),
            s => panic!("loader error {s:?}"),           // lib.rs:45-46: unwrap() of Field / Group / InvalidPoint errors
        }
    }
    /// One batch over many keys (`bn254_groth16_verify_batch_keys`): proof `i` is verified against `keys[key_index[i]]`; its inputs are the first
    /// `32 * num_public(that key)` bytes of row `i` of `public_inputs` (`input_stride` bytes per row, at least 32 x the largest input count of the list).  A key may
    /// occur more than once in `keys`; keys with more than 16 public inputs and an index outside the list are refused (`BN254_E_BAD_ARG`).  `FLAG_RLC` is accepted
    /// and ignored.  The device state of the list is cached by the library under the handles in order.
    pub fn verify_batch_keys(keys: &[&PreparedGroth16Vk], key_index: &[u32], proofs: &[u8], proof_stride: usize, public_inputs: &[u8], input_stride: usize, device: i32,
                             flags: u32) -> Result<Vec<Status>, Error> {
        let n = key_index.len();
        assert!(proof_stride >= g16_min_stride(flags) && proofs.len() >= n * proof_stride && public_inputs.len() >= n * input_stride);
        let h: Vec<*const sys::Bn254G16Pvk> = keys.iter().map(|k| k.h as *const sys::Bn254G16Pvk).collect();
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_groth16_verify_batch_keys(h.as_ptr() as *mut *const sys::Bn254G16Pvk, h.len(), key_index.as_ptr(), proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), input_stride, n,
                                                            st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// Tables and workspace of a key list ahead of its first batch of up to `n` proofs (`bn254_groth16_reserve_keys`).
    pub fn reserve_keys(keys: &[&PreparedGroth16Vk], n: usize, device: i32) -> Result<(), Error> {
        let h: Vec<*const sys::Bn254G16Pvk> = keys.iter().map(|k| k.h as *const sys::Bn254G16Pvk).collect();
        check(unsafe { sys::bn254_groth16_reserve_keys(h.as_ptr() as *mut *const sys::Bn254G16Pvk, h.len(), n, device) })
    }
    /// New: N proofs against one key, one `Status` each; nothing panics.
    pub fn verify_batch(proofs: &[&[u8]], vk: &[u8], public_inputs: &[&[[u8; 32]]]) -> Result<Vec<Status>, Error> {
        Self::verify_batch_opts(proofs, vk, public_inputs, false)
    }
    /// `verify_batch` with the proof layout as an option: `compressed` = gnark's compressed proofs (its default `WriteTo` form, 128 bytes: A | B | C),
    /// decompressed on the device (`FLAG_COMPRESSED_PROOFS`); a proof that does not decompress is `Status::Malformed`.
    pub fn verify_batch_opts(proofs: &[&[u8]], vk: &[u8], public_inputs: &[&[[u8; 32]]], compressed: bool) -> Result<Vec<Status>, Error> {
        assert_eq!(proofs.len(), public_inputs.len());
        let pvk = PreparedGroth16Vk::new(vk, VkMode::Reference)?;
        let (flags, min_len) = if compressed { (FLAG_COMPRESSED_PROOFS, 128) } else { (0, 256) };
        let (buf, stride) = flatten(proofs, min_len);
        let n_public = public_inputs.first().map_or(0, |x| x.len());
        assert!(public_inputs.iter().all(|x| x.len() == n_public), "one input count per batch (a wrong count is a per-key error: InputLen for every proof)");
        let inputs: Vec<u8> = public_inputs.iter().flat_map(|xs| xs.iter().flatten().copied()).collect();
        let mut st = pvk.verify_batch_raw(&buf, stride, &inputs, n_public, proofs.len(), 0, flags)?;
        for (s, p) in st.iter_mut().zip(proofs) { if p.len() < min_len { *s = Status::Malformed; } }   // a slice-index panic in the reference
        Ok(st)
    }
}

/// `load_plonk_verifying_key_from_bytes` (`plonk/converter.rs:18-119`) + the key-side tables, done once.
pub struct PreparedPlonkVk { h: *mut sys::Bn254PlonkPvk }
unsafe impl Send for PreparedPlonkVk {}
unsafe impl Sync for PreparedPlonkVk {}     // several threads may call verify_batch on one key: the library hands out per-call contexts
impl PreparedPlonkVk {
    pub fn new(vk: &[u8]) -> Result<Self, Error> {
        let mut h = core::ptr::null_mut();
        check(unsafe { sys::bn254_plonk_vk_prepare(vk.as_ptr(), vk.len(), &mut h) })?;
        Ok(Self { h })
    }
    pub fn num_public(&self) -> usize { unsafe { sys::bn254_plonk_vk_num_public(self.h) } }
    /// Allocations ahead of the first batch of up to `n` proofs (`proof_stride` > 0: also the pinned staging of the host-buffer entry); see the header for the footprint.
    pub fn reserve(&self, n: usize, proof_stride: usize, device: i32) -> Result<(), Error> { check(unsafe { sys::bn254_plonk_reserve(self.h, n, proof_stride, device) }) }
    /// Device memory this key's contexts hold on `device` (bytes) and how many contexts hold any.
    pub fn footprint(&self, device: i32) -> Result<(usize, i32), Error> {
        let (mut bytes, mut ctx) = (0usize, 0);
        check(unsafe { sys::bn254_plonk_footprint(self.h, device, &mut bytes, &mut ctx) })?;
        Ok((bytes, ctx))
    }
    pub fn verify_batch_raw(&self, proofs: &[u8], proof_stride: usize, public_inputs: &[u8], n_public: usize, n: usize, device: i32) -> Result<Vec<Status>, Error> {
        self.verify_batch_flags(proofs, proof_stride, public_inputs, n_public, n, device, 0)
    }
    /// `flags`: `sys::BN254_FLAG_RLC` batches the pairing checks of a pass across proofs (one check per 64 proofs, exact fallback on the groups that fail;
    /// honoured from 8192 proofs per pass).  Same status bytes as `verify_batch_raw`.
    pub fn verify_batch_flags(&self, proofs: &[u8], proof_stride: usize, public_inputs: &[u8], n_public: usize, n: usize, device: i32, flags: u32) -> Result<Vec<Status>, Error> {
        assert!(proofs.len() >= n * proof_stride && public_inputs.len() >= n * n_public * 32);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_plonk_verify_batch_flags(self.h, proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), n_public, n, st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// SP1 proofs from their public values, as `PreparedGroth16Vk::verify_sp1_batch`; `flags`: `sys::BN254_FLAG_RLC` only.
    pub fn verify_sp1_batch(&self, proofs: &[u8], proof_stride: usize, vkey_hashes: &[[u8; 32]], public_values: &[&[u8]], device: i32, flags: u32) -> Result<Vec<Status>, Error> {
        let n = public_values.len();
        assert!(proofs.len() >= n * proof_stride);
        let (pv, offs, vk, stride) = sp1_buffers(vkey_hashes, public_values);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_sp1_plonk_verify_batch(self.h, proofs.as_ptr(), proof_stride, vk.as_ptr(), stride, pv.as_ptr(), offs.as_ptr(), n, st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// The same over the GPUs selected by `device_mask` (contiguous shards, one host thread per device: SURVEY.md section 8(e)).
    pub fn verify_batch_multi_raw(&self, proofs: &[u8], proof_stride: usize, public_inputs: &[u8], n_public: usize, n: usize, device_mask: u64, flags: u32) -> Result<Vec<Status>, Error> {
        assert!(proofs.len() >= n * proof_stride && public_inputs.len() >= n * n_public * 32);
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_plonk_verify_batch_multi(self.h, proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), n_public, n, st.as_mut_ptr(), device_mask, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// Proofs, inputs and status bytes in device memory.  Host-synchronous: waits for `hip_stream`, returns when the status bytes are in `d_status`.
    /// # Safety
    /// The three device pointers must be valid for the sizes implied by `n`, `proof_stride`, `n_public` for the duration of the call.
    pub unsafe fn verify_batch_device(&self, d_proofs: *const c_void, proof_stride: usize, d_inputs: *const c_void, n_public: usize, n: usize, d_status: *mut c_void, device: i32,
                                      hip_stream: *mut c_void, flags: u32) -> Result<(), Error> {
        check(sys::bn254_plonk_verify_batch_device(self.h, d_proofs, proof_stride, d_inputs, n_public, n, d_status, device, hip_stream, flags))
    }
    /// Durations (ms) of the first sub-batch of the batch that finished last on `device` (slots: `bn254_plonk_last_timing` in the header) and the lanes of its two MSM launches.
    pub fn last_timing(&self, device: i32) -> Result<([f32; sys::BN254_PLONK_NUM_TIMINGS], [usize; 2]), Error> {
        let (mut ms, mut lanes) = ([0f32; sys::BN254_PLONK_NUM_TIMINGS], [0usize; 2]);
        check(unsafe { sys::bn254_plonk_last_timing(self.h, device, ms.as_mut_ptr(), lanes.as_mut_ptr()) })?;
        Ok((ms, lanes))
    }
}
impl Drop for PreparedPlonkVk { fn drop(&mut self) { unsafe { sys::bn254_plonk_vk_free(self.h) } } }

/// At most this many (G1, G2) pairs per item of `pairing_check_batch`.
pub const PAIRING_MAX_PAIRS: usize = sys::BN254_PAIRING_MAX_PAIRS as usize;
/// Bytes of one pair: G1 `x | y` (64), then G2 `x.c1 | x.c0 | y.c1 | y.c0` (128), 32-byte big-endian coordinates -- gnark's order and EIP-197's.
pub const PAIRING_PAIR_LEN: usize = sys::BN254_PAIRING_PAIR_LEN as usize;

/// `bn::pairing_batch(&[(G1, G2)])` checked against 1, for `n` items at once on the GPU (`bn254_pairing_check_batch`): item `i` holds `n_pairs` records of
/// `PAIRING_PAIR_LEN` bytes at `pairs[i * item_stride..]`; an all-zero point is the identity.  Per item `Status::Accept` (the product of its pairings is 1),
/// `Status::Reject`, or what `AffineG1::new` / `AffineG2::new` refuse: `NotMember`, `NotOnCurve`, `NotInSubgroup` (the header has the order).
pub fn pairing_check_batch(pairs: &[u8], item_stride: usize, n_pairs: usize, n: usize, device: i32) -> Result<Vec<Status>, Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "pairing_check_batch: n_pairs is 1..=8 and the buffer holds n items of item_stride bytes".into() };
    if n_pairs < 1 || n_pairs > PAIRING_MAX_PAIRS || item_stride < PAIRING_PAIR_LEN * n_pairs { return Err(short); }
    if n > 0 && (n - 1).checked_mul(item_stride).and_then(|b| b.checked_add(PAIRING_PAIR_LEN * n_pairs)).map_or(true, |b| pairs.len() < b) { return Err(short); }
    let mut status = vec![0u8; n];
    check(unsafe { sys::bn254_pairing_check_batch(pairs.as_ptr(), item_stride, n_pairs, n, status.as_mut_ptr(), device as c_int) })?;
    Ok(status.into_iter().map(Status::from).collect())
}
/// Bytes of a prepared G2 record (`g2_prepare`): a header, the affine point and its 88 lines.  Valid only for the layout version that wrote it.
pub const G2_PREPARED_LEN: usize = sys::BN254_G2_PREPARED_LEN;
/// Bytes of a shared position of a packed item: G1 `x | y` alone.
pub const PAIRING_G1_LEN: usize = sys::BN254_PAIRING_G1_LEN;

/// The prepared record of the G2 point `x.c1 | x.c0 | y.c1 | y.c0` (all zero: the identity) for the positions of a batch that share it (`bn254_g2_prepare`; host
/// work, no device): `Ok(record)`, or `Err(Status::NotMember | NotOnCurve | NotInSubgroup)` as the inner error when the point is refused.
pub fn g2_prepare(g2: &[u8; 128]) -> Result<Result<Vec<u8>, Status>, Error> {
    let mut out = vec![0u8; G2_PREPARED_LEN];
    let mut st = 0u8;
    check(unsafe { sys::bn254_g2_prepare(g2.as_ptr(), out.as_mut_ptr(), &mut st) })?;
    Ok(if st == sys::BN254_ACCEPT { Ok(out) } else { Err(Status::from(st)) })
}
/// Bytes of a packed item of `n_pairs` positions: `PAIRING_G1_LEN` per position whose bit of `shared_mask` is set, `PAIRING_PAIR_LEN` per other one.
pub fn pairing_packed_len(n_pairs: usize, shared_mask: u32) -> usize {
    (0..n_pairs).map(|j| if (shared_mask >> j) & 1 == 1 { PAIRING_G1_LEN } else { PAIRING_PAIR_LEN }).sum()
}
/// `pairing_check_batch` for items in which the G2 point of every position `j` with bit `j` of `shared_mask` set is the same for the whole batch
/// (`bn254_pairing_check_batch_shared`): `prepared` holds the records of those positions (`g2_prepare`) in ascending position order, and the items are packed --
/// a shared position holds its G1 point alone.  The statuses are those of `pairing_check_batch` on the expanded items.
pub fn pairing_check_batch_shared(items: &[u8], item_stride: usize, n_pairs: usize, shared_mask: u32, prepared: &[u8], n: usize, device: i32) -> Result<Vec<Status>, Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "pairing_check_batch_shared: n_pairs is 1..=8, shared_mask has bits below n_pairs only, prepared holds a record per shared position and the buffer holds n packed items of item_stride bytes".into() };
    if n_pairs < 1 || n_pairs > PAIRING_MAX_PAIRS || (shared_mask >> n_pairs) != 0 { return Err(short); }
    let packed = pairing_packed_len(n_pairs, shared_mask);
    if item_stride < packed || prepared.len() < G2_PREPARED_LEN * shared_mask.count_ones() as usize { return Err(short); }
    if n > 0 && (n - 1).checked_mul(item_stride).and_then(|b| b.checked_add(packed)).map_or(true, |b| items.len() < b) { return Err(short); }
    let mut status = vec![0u8; n];
    check(unsafe { sys::bn254_pairing_check_batch_shared(items.as_ptr(), item_stride, n_pairs, shared_mask as core::ffi::c_uint, prepared.as_ptr(), n, status.as_mut_ptr(), device as c_int) })?;
    Ok(status.into_iter().map(Status::from).collect())
}
/// `pairing_check_batch_shared` with a flags word (`bn254_pairing_check_batch_flags`): `flags` may hold `FLAG_RLC` only, 0 is the exact entry, and `shared_mask == 0`
/// with an empty `prepared` is the all-variable item.  With the flag honoured (launches of `pairing_rlc_params()` items or more of a shape without a variable position; any other launch is the exact one) the 64 items of a wavefront are
/// checked jointly under fresh random 128-bit weights: the statuses are those of the exact entry except that a false `Accept` has probability about 2^-127 per item,
/// and the call synchronises once per launch.
pub fn pairing_check_batch_flags(items: &[u8], item_stride: usize, n_pairs: usize, shared_mask: u32, prepared: &[u8], n: usize, device: i32, flags: u32) -> Result<Vec<Status>, Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "pairing_check_batch_flags: n_pairs is 1..=8, shared_mask has bits below n_pairs only, prepared holds a record per shared position and the buffer holds n packed items of item_stride bytes".into() };
    if n_pairs < 1 || n_pairs > PAIRING_MAX_PAIRS || (shared_mask >> n_pairs) != 0 { return Err(short); }
    let packed = pairing_packed_len(n_pairs, shared_mask);
    if item_stride < packed || prepared.len() < G2_PREPARED_LEN * shared_mask.count_ones() as usize { return Err(short); }
    if n > 0 && (n - 1).checked_mul(item_stride).and_then(|b| b.checked_add(packed)).map_or(true, |b| items.len() < b) { return Err(short); }
    let mut status = vec![0u8; n];
    let recs = if shared_mask == 0 { core::ptr::null() } else { prepared.as_ptr() };
    check(unsafe { sys::bn254_pairing_check_batch_flags(items.as_ptr(), item_stride, n_pairs, shared_mask as core::ffi::c_uint, recs, n, status.as_mut_ptr(), device as c_int, flags as core::ffi::c_uint) })?;
    Ok(status.into_iter().map(Status::from).collect())
}
/// `bn254_pairing_check_batch_flags_device` on device pointers: enqueues on `hip_stream`; a launch that honours `FLAG_RLC` synchronises the stream once.
///
/// # Safety
/// The pointers must be device memory of the sizes the call implies (`d_prepared` 4-byte aligned) and stay valid until the stream has run the work.
pub unsafe fn pairing_check_batch_flags_device(d_items: *const core::ffi::c_void, item_stride: usize, n_pairs: usize, shared_mask: u32, d_prepared: *const core::ffi::c_void, n: usize,
                                               d_status: *mut core::ffi::c_void, device: i32, hip_stream: *mut core::ffi::c_void, flags: u32) -> Result<(), Error> {
    check(sys::bn254_pairing_check_batch_flags_device(d_items, item_stride, n_pairs, shared_mask as core::ffi::c_uint, d_prepared, n, d_status, device as c_int, hip_stream, flags as core::ffi::c_uint))
}
/// `FLAG_RLC` on the pairing batch is honoured from `rlc_min` items per launch on (`bn254_set_pairing_rlc_params`; never below 64; negative: unchanged).
pub fn set_pairing_rlc_params(rlc_min: i64) { unsafe { sys::bn254_set_pairing_rlc_params(rlc_min as core::ffi::c_long) } }
/// The knob as it is now (`bn254_pairing_rlc_params`).
pub fn pairing_rlc_params() -> Result<i64, Error> {
    let mut out: [core::ffi::c_long; 1] = [0];
    check(unsafe { sys::bn254_pairing_rlc_params(out.as_mut_ptr()) })?;
    Ok(out[0] as i64)
}
/// (launches that ran the joint check, groups they checked, groups that failed, launches on the exact path)  (`bn254_pairing_rlc_state`).
pub fn pairing_rlc_state() -> Result<(u64, u64, u64, u64), Error> {
    let mut out = [0u64; 4];
    check(unsafe { sys::bn254_pairing_rlc_state(out.as_mut_ptr()) })?;
    Ok((out[0], out[1], out[2], out[3]))
}
/// Makes `device` ready for pairing batches of `n` items (its self-test at first use, the workspace).
pub fn pairing_reserve(n: usize, device: i32) -> Result<(), Error> { check(unsafe { sys::bn254_pairing_reserve(n, device as c_int) }) }
/// Launches of up to `coop_max` items of a pairing batch take the cooperative twelve-lane form (`bn254_set_pairing_params`; 0: always the lane form; clamped to
/// 30 720; negative: unchanged).
pub fn set_pairing_params(coop_max: i64) { unsafe { sys::bn254_set_pairing_params(coop_max as core::ffi::c_long) } }
/// The knob as it is now (`bn254_pairing_params`).
pub fn pairing_params() -> Result<i64, Error> {
    let mut out: [core::ffi::c_long; 1] = [0];
    check(unsafe { sys::bn254_pairing_params(out.as_mut_ptr()) })?;
    Ok(out[0] as i64)
}
/// Launches of pairing batches enqueued so far by this process: (in the cooperative form, in the lane form)  (`bn254_pairing_state`).
pub fn pairing_state() -> Result<(u64, u64), Error> {
    let mut out = [0u64; 2];
    check(unsafe { sys::bn254_pairing_state(out.as_mut_ptr()) })?;
    Ok((out[0], out[1]))
}

/// Bytes of a KZG opening: commitment `x | y`, quotient `x | y`, point `z`, claimed value `y`, 32-byte big-endian each.
pub const KZG_OPENING_LEN: usize = sys::BN254_KZG_OPENING_LEN;
/// Bytes of a KZG key (`kzg_key_prepare`): plain data -- a header, g1 and the prepared records of g2 and tau_g2.  Valid only for the layout version that wrote it.
pub const KZG_KEY_LEN: usize = sys::BN254_KZG_KEY_LEN;

/// The key of a KZG setup (`bn254_kzg_key_prepare`; host work, no device): `Ok(key)`, or the first failure over g1, g2, tau_g2 as the inner error.
pub fn kzg_key_prepare(g1: &[u8; 64], g2: &[u8; 128], tau_g2: &[u8; 128]) -> Result<Result<Vec<u8>, Status>, Error> {
    let mut out = vec![0u8; KZG_KEY_LEN];
    let mut st = 0u8;
    check(unsafe { sys::bn254_kzg_key_prepare(g1.as_ptr(), g2.as_ptr(), tau_g2.as_ptr(), out.as_mut_ptr(), &mut st) })?;
    Ok(if st == sys::BN254_ACCEPT { Ok(out) } else { Err(Status::from(st)) })
}
/// Batch verification of `n` KZG openings of `stride` bytes each (`bn254_kzg_verify_batch`): `Accept` where `e(C - y g1 + z H, g2) e(-H, tau_g2) == 1`, `Reject` where
/// it is not, or the loader error.  `flags`: `FLAG_STRICT_SCALARS`, `FLAG_RLC` (the joint check over groups of 64 openings, honoured from `set_kzg_params`' `rlc_min`
/// openings per launch on: the same statuses except for a false accept with probability about 2^-127).
pub fn kzg_verify_batch(key: &[u8], openings: &[u8], stride: usize, n: usize, device: i32, flags: u32) -> Result<Vec<Status>, Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "kzg_verify_batch: the key holds KZG_KEY_LEN bytes, stride is at least KZG_OPENING_LEN and the buffer holds n openings of stride bytes".into() };
    if key.len() < KZG_KEY_LEN || stride < KZG_OPENING_LEN { return Err(short); }
    if n > 0 && (n - 1).checked_mul(stride).and_then(|b| b.checked_add(KZG_OPENING_LEN)).map_or(true, |b| openings.len() < b) { return Err(short); }
    let mut status = vec![0u8; n];
    check(unsafe { sys::bn254_kzg_verify_batch(key.as_ptr(), openings.as_ptr(), stride, n, status.as_mut_ptr(), device as c_int, flags as core::ffi::c_uint) })?;
    Ok(status.into_iter().map(Status::from).collect())
}
/// Makes `device` ready for KZG batches of `n` openings (its self-test at first use, the workspace and the buffers of the G1 walk).
pub fn kzg_reserve(n: usize, device: i32) -> Result<(), Error> { check(unsafe { sys::bn254_kzg_reserve(n, device as c_int) }) }
/// The most digests a batch-opening record holds, and the most bytes of caller data (`kzg_verify_folded_batch`).
pub const KZG_FOLD_MAX_DIGESTS: usize = sys::BN254_KZG_FOLD_MAX_DIGESTS as usize;
pub const KZG_FOLD_MAX_DATA: usize = sys::BN254_KZG_FOLD_MAX_DATA as usize;
/// Bytes of a batch-opening record: `D_0 .. D_{k-1}` (64 each), `H` (64), `z` (32), `y_0 .. y_{k-1}` (32 each), then `data_len` bytes of caller data.
pub const fn kzg_fold_len(n_digests: usize, data_len: usize) -> usize { 96 + 96 * n_digests + data_len }
/// Batch verification of `n` KZG batch-opening proofs (`bn254_kzg_verify_folded_batch`; the reference's `kzg::fold_proof`): `n_digests` commitments opened at one
/// point with one quotient, folded with the challenge of the SHA-256 transcript over the point, the digests, the claimed values and the data.  `Accept` where the
/// folded opening verifies, `Reject` where it does not, or the loader error; `flags` as `kzg_verify_batch`.
pub fn kzg_verify_folded_batch(key: &[u8], records: &[u8], stride: usize, n: usize, n_digests: usize, data_len: usize, device: i32, flags: u32) -> Result<Vec<Status>, Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "kzg_verify_folded_batch: the key holds KZG_KEY_LEN bytes, n_digests is 1 ..= KZG_FOLD_MAX_DIGESTS, data_len at most KZG_FOLD_MAX_DATA, stride at least kzg_fold_len(n_digests, data_len) and the buffer holds n records of stride bytes".into() };
    if key.len() < KZG_KEY_LEN || n_digests < 1 || n_digests > KZG_FOLD_MAX_DIGESTS || data_len > KZG_FOLD_MAX_DATA { return Err(short); }
    let len = kzg_fold_len(n_digests, data_len);
    if stride < len { return Err(short); }
    if n > 0 && (n - 1).checked_mul(stride).and_then(|b| b.checked_add(len)).map_or(true, |b| records.len() < b) { return Err(short); }
    let mut status = vec![0u8; n];
    check(unsafe { sys::bn254_kzg_verify_folded_batch(key.as_ptr(), records.as_ptr(), stride, n, n_digests, data_len, status.as_mut_ptr(), device as c_int, flags as core::ffi::c_uint) })?;
    Ok(status.into_iter().map(Status::from).collect())
}
/// Makes `device` ready for batches of `n` records of `n_digests` digests (`bn254_kzg_fold_reserve`).
pub fn kzg_fold_reserve(n: usize, n_digests: usize, device: i32) -> Result<(), Error> { check(unsafe { sys::bn254_kzg_fold_reserve(n, n_digests, device as c_int) }) }
/// `FLAG_RLC` is honoured from `rlc_min` openings per launch on (`bn254_set_kzg_params`; never below 64; negative: unchanged).
pub fn set_kzg_params(rlc_min: i64) { unsafe { sys::bn254_set_kzg_params(rlc_min as core::ffi::c_long) } }
/// The knob as it is now (`bn254_kzg_params`).
pub fn kzg_params() -> Result<i64, Error> {
    let mut out: [core::ffi::c_long; 1] = [0];
    check(unsafe { sys::bn254_kzg_params(out.as_mut_ptr()) })?;
    Ok(out[0] as i64)
}
/// (launches that ran the joint check, groups they checked, groups that failed, launches on the exact path)  (`bn254_kzg_state`).
pub fn kzg_state() -> Result<(u64, u64, u64, u64), Error> {
    let mut out = [0u64; 4];
    check(unsafe { sys::bn254_kzg_state(out.as_mut_ptr()) })?;
    Ok((out[0], out[1], out[2], out[3]))
}

/// The most variable, unit and shared terms of a `g1_msm_batch` item.
pub const G1_MSM_MAX_VAR: usize = sys::BN254_G1_MSM_MAX_VAR as usize;
pub const G1_MSM_MAX_UNIT: usize = sys::BN254_G1_MSM_MAX_UNIT as usize;
pub const G1_MSM_MAX_SHARED: usize = sys::BN254_G1_MSM_MAX_SHARED as usize;
/// Bytes of an item: `n_var` pairs (point `x | y`, scalar), `n_unit` points, `n_shared` scalars, 32-byte big-endian fields (`BN254_G1_MSM_ITEM_LEN`).
pub const fn g1_msm_item_len(n_var: usize, n_unit: usize, n_shared: usize) -> usize { 96 * n_var + 64 * n_unit + 32 * n_shared }
/// The shared bases of `g1_msm_batch` on one device (`bn254_g1_bases_prepare`): their window tables live in device memory until the value is dropped, which waits
/// for the device first.
pub struct G1Bases { handle: *mut core::ffi::c_void, device: i32 }
unsafe impl Send for G1Bases {}
unsafe impl Sync for G1Bases {}
impl G1Bases {
    /// `Ok(bases)` from 1 ..= `G1_MSM_MAX_SHARED` points of 64 bytes, or the first failure over the points as the inner error.
    pub fn prepare(points: &[u8], device: i32) -> Result<Result<G1Bases, Status>, Error> {
        if points.is_empty() || points.len() % 64 != 0 || points.len() / 64 > G1_MSM_MAX_SHARED {
            return Err(Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "G1Bases::prepare: 1 ..= G1_MSM_MAX_SHARED points of 64 bytes".into() });
        }
        let mut handle: *mut core::ffi::c_void = core::ptr::null_mut();
        let mut st = 0u8;
        check(unsafe { sys::bn254_g1_bases_prepare(points.as_ptr(), points.len() / 64, device as c_int, &mut handle, &mut st) })?;
        Ok(if st == sys::BN254_ACCEPT && !handle.is_null() { Ok(G1Bases { handle, device }) } else { Err(Status::from(st)) })
    }
    /// The number of points (`bn254_g1_bases_count`).
    pub fn len(&self) -> usize { unsafe { sys::bn254_g1_bases_count(self.handle) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
    /// The device the tables live on.
    pub fn device(&self) -> i32 { self.device }
}
impl Drop for G1Bases {
    fn drop(&mut self) { unsafe { sys::bn254_g1_bases_free(self.handle) } }
}
/// Batch G1 multi-scalar multiplication (`bn254_g1_msm_batch`): per item `sum k_t P_t + sum U_t + sum c_j B_j` as 64 bytes `x | y` (zero: the identity, or an item
/// that ended in an error) and its status (`Accept`, or the loader error).  `bases` is needed exactly when `n_shared > 0`.  `flags`: `FLAG_STRICT_SCALARS`.
pub fn g1_msm_batch(items: &[u8], stride: usize, n_var: usize, n_unit: usize, n_shared: usize, bases: Option<&G1Bases>, n: usize, device: i32, flags: u32) -> Result<(Vec<u8>, Vec<Status>), Error> {
    let short = Error::Infrastructure { code: sys::BN254_E_BAD_ARG, message: "g1_msm_batch: a shape within the limits with a term, stride at least g1_msm_item_len(n_var, n_unit, n_shared) and a buffer of n items of stride bytes".into() };
    if n_var > G1_MSM_MAX_VAR || n_unit > G1_MSM_MAX_UNIT || n_shared > G1_MSM_MAX_SHARED || n_var + n_unit + n_shared == 0 { return Err(short); }
    let len = g1_msm_item_len(n_var, n_unit, n_shared);
    if stride < len { return Err(short); }
    if n > 0 && (n - 1).checked_mul(stride).and_then(|b| b.checked_add(len)).map_or(true, |b| items.len() < b) { return Err(short); }
    let mut out = vec![0u8; 64 * n];
    let mut status = vec![0u8; n];
    let handle = bases.map_or(core::ptr::null(), |b| b.handle as *const core::ffi::c_void);
    check(unsafe { sys::bn254_g1_msm_batch(items.as_ptr(), stride, n_var, n_unit, n_shared, handle, n, out.as_mut_ptr(), status.as_mut_ptr(), device as c_int, flags as core::ffi::c_uint) })?;
    Ok((out, status.into_iter().map(Status::from).collect()))
}
/// `bn254_g1_msm_batch_device` on device pointers: enqueues on `hip_stream` and returns; `d_out` receives 64 n bytes, `d_status` n.
///
/// # Safety
/// The pointers must be device memory of the sizes the call implies and stay valid until the stream has run the work.
pub unsafe fn g1_msm_batch_device(d_items: *const core::ffi::c_void, stride: usize, n_var: usize, n_unit: usize, n_shared: usize, bases: Option<&G1Bases>, n: usize,
                                  d_out: *mut core::ffi::c_void, d_status: *mut core::ffi::c_void, device: i32, hip_stream: *mut core::ffi::c_void, flags: u32) -> Result<(), Error> {
    let handle = bases.map_or(core::ptr::null(), |b| b.handle as *const core::ffi::c_void);
    check(sys::bn254_g1_msm_batch_device(d_items, stride, n_var, n_unit, n_shared, handle, n, d_out, d_status, device as c_int, hip_stream, flags as core::ffi::c_uint))
}
/// Makes `device` ready for batches of `n` items of a shape: a later `g1_msm_batch_device` of up to `n` such items only enqueues (`bn254_g1_msm_reserve`).
pub fn g1_msm_reserve(n: usize, n_var: usize, n_unit: usize, n_shared: usize, device: i32) -> Result<(), Error> {
    check(unsafe { sys::bn254_g1_msm_reserve(n, n_var, n_unit, n_shared, device as c_int) })
}

/// The library this crate was generated for?  (`bn254_abi_version`: bumped whenever a function changes its arguments, an array its length or a slot its meaning.)
pub fn abi_matches() -> bool { unsafe { sys::bn254_abi_version() == sys::BN254_ABI_VERSION } }

pub struct PlonkVerifier;
impl PlonkVerifier {
    /// `PlonkVerifier::verify` (`lib.rs:69-74`).
    pub fn verify(proof: &[u8], vk: &[u8], public_inputs: &[[u8; 32]]) -> Result<bool, PlonkError> {
        let inputs: Vec<u8> = public_inputs.iter().flatten().copied().collect();
        let mut st = 0u8;
        let rc = unsafe { sys::bn254_plonk_verify(proof.as_ptr(), proof.len(), vk.as_ptr(), vk.len(), inputs.as_ptr(), public_inputs.len(), &mut st) };
        check(rc).expect("bn254 infrastructure error");
        match Status::from(st) {
            Status::Accept => Ok(true),                                       // never Ok(false): plonk/verify.rs:316
            Status::InputLen => Err(PlonkError::InvalidWitness),              // plonk/verify.rs:57-59
            Status::OpeningMismatch => Err(PlonkError::OpeningPolyMismatch),  // plonk/verify.rs:212-214
            Status::PairingFailed => Err(PlonkError::PairingCheckFailed),     // plonk/kzg.rs:185-187
            Status::Bsb22Mismatch => Err(PlonkError::Bsb22CommitmentMismatch),// plonk/verify.rs:52-54
            Status::Inverse => Err(PlonkError::InverseNotFound),              // plonk/verify.rs:106
            s => panic!("loader error {s:?}"),                                // lib.rs:70-71
        }
    }
    /// One batch over many keys (`bn254_plonk_verify_batch_keys`): proof `i` is verified against `keys[key_index[i]]`; its inputs are the first
    /// `32 * num_public(that key)` bytes of row `i` of `public_inputs` (`input_stride` bytes per row, at least 32 x the largest input count of the list).  At most 256
    /// keys, all with the same number of BSB22 commitments; a key may occur more than once; an index outside the list is refused (`BN254_E_BAD_ARG`).
    /// `BN254_FLAG_RLC` is accepted and ignored.  The device state of the list is cached by the library under the handles in order.
    pub fn verify_batch_keys(keys: &[&PreparedPlonkVk], key_index: &[u32], proofs: &[u8], proof_stride: usize, public_inputs: &[u8], input_stride: usize, device: i32,
                             flags: u32) -> Result<Vec<Status>, Error> {
        let n = key_index.len();
        assert!(proofs.len() >= n * proof_stride && public_inputs.len() >= n * input_stride);
        let h: Vec<*const sys::Bn254PlonkPvk> = keys.iter().map(|k| k.h as *const sys::Bn254PlonkPvk).collect();
        let mut st = vec![0u8; n];
        check(unsafe { sys::bn254_plonk_verify_batch_keys(h.as_ptr() as *mut *const sys::Bn254PlonkPvk, h.len(), key_index.as_ptr(), proofs.as_ptr(), proof_stride, public_inputs.as_ptr(), input_stride, n,
                                                          st.as_mut_ptr(), device, flags) })?;
        Ok(st.into_iter().map(Status::from).collect())
    }
    /// Members' tables, contexts and staging of a key list ahead of its first batch of up to `n` proofs of `proof_stride` bytes (`bn254_plonk_reserve_keys`).
    pub fn reserve_keys(keys: &[&PreparedPlonkVk], n: usize, proof_stride: usize, device: i32) -> Result<(), Error> {
        let h: Vec<*const sys::Bn254PlonkPvk> = keys.iter().map(|k| k.h as *const sys::Bn254PlonkPvk).collect();
        check(unsafe { sys::bn254_plonk_reserve_keys(h.as_ptr() as *mut *const sys::Bn254PlonkPvk, h.len(), n, proof_stride, device) })
    }
    /// Counters of the list's cached state on `device` (`bn254_plonk_keys_state`): passes that ran the joint check of `BN254_FLAG_RLC`, the groups they checked,
    /// the groups that failed, passes whose per-proof pairing check ran in the cooperative form.
    pub fn keys_state(keys: &[&PreparedPlonkVk], device: i32) -> Result<[u64; 4], Error> {
        let h: Vec<*const sys::Bn254PlonkPvk> = keys.iter().map(|k| k.h as *const sys::Bn254PlonkPvk).collect();
        let mut out = [0u64; 4];
        check(unsafe { sys::bn254_plonk_keys_state(h.as_ptr() as *mut *const sys::Bn254PlonkPvk, h.len(), device, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// Passes of up to `coop_max` slots of a batch over a key list take the cooperative pairing form (`bn254_set_plonk_keys_params`; 0: always the lane form).
    pub fn set_keys_params(coop_max: i64) { unsafe { sys::bn254_set_plonk_keys_params(coop_max as core::ffi::c_long) } }
    /// The pass size from which `BN254_FLAG_RLC` is honoured, on one key and over a list (`bn254_set_plonk_rlc_params`; never below 64).
    pub fn set_rlc_params(min_pass: i64) { unsafe { sys::bn254_set_plonk_rlc_params(min_pass as core::ffi::c_long) } }
    pub fn verify_batch(proofs: &[&[u8]], vk: &[u8], public_inputs: &[&[[u8; 32]]]) -> Result<Vec<Status>, Error> {
        assert_eq!(proofs.len(), public_inputs.len());
        let pvk = PreparedPlonkVk::new(vk)?;
        let (buf, stride) = flatten(proofs, 516);
        let n_public = public_inputs.first().map_or(0, |x| x.len());
        assert!(public_inputs.iter().all(|x| x.len() == n_public), "one input count per batch (a wrong count is a per-key error: InputLen for every proof)");
        let inputs: Vec<u8> = public_inputs.iter().flat_map(|xs| xs.iter().flatten().copied()).collect();
        let mut st = pvk.verify_batch_raw(&buf, stride, &inputs, n_public, proofs.len(), 0)?;
        // a proof shorter than its own layout is a slice-index panic in the reference (plonk/converter.rs:121-178); zero-padded to the stride it would parse as something else
        for (s, p) in st.iter_mut().zip(proofs) { if p.len() < plonk_layout_len(p) { *s = Status::Malformed; } }
        Ok(st)
    }
}

/// Bytes `load_plonk_proof_from_bytes` reads of a proof that starts like `p` (`plonk/converter.rs:121-178`): 8 points, u32 count + claimed values, the second opening
/// (point, value, u32 count) and the BSB22 commitments; `usize::MAX` when `p` ends before a count can be read.
fn plonk_layout_len(p: &[u8]) -> usize {
    let be32 = |o: usize| p.get(o..o + 4).map(|b| u32::from_be_bytes([b[0], b[1], b[2], b[3]]) as usize);
    let Some(n_claimed) = be32(512) else { return usize::MAX };
    let off = 516 + 32 * n_claimed;
    let Some(n_bsb) = be32(off + 96) else { return usize::MAX };
    off + 100 + 64 * n_bsb
}

/// The contiguous shard of rank `r` of `world` for a batch of `n` (the rule of `bn254_shard_plan` and of the multi-process job).
pub fn shard_bounds(n: usize, world: usize, r: usize) -> (usize, usize) {
    let (base, rem) = (n / world, n % world);
    (r * base + r.min(rem), base + usize::from(r < rem))
}
/// Multi-process job, one process per GPU: one `ncclAllGather` of the ranks' status bytes (RCCL over xGMI); `comm` is the host's `ncclComm_t`.
/// # Safety
/// Device pointers and the communicator must be valid; `d_full` holds `n` bytes, `d_scratch` `world * ceil(n / world)` when `n % world != 0`.
pub unsafe fn status_all_gather(comm: *mut c_void, world: i32, rank: i32, d_local: *const c_void, n: usize, d_full: *mut c_void, d_scratch: *mut c_void, hip_stream: *mut c_void) -> Result<(), Error> {
    check(sys::bn254_status_all_gather(comm, world, rank, d_local, n, d_full, d_scratch, hip_stream))
}

#[cfg(test)]
mod tests {
    //! Needs an MI355X (the library has no CPU path) and the repository's `tests/golden/` next to `rust/`.
    use super::*;
    use std::{fs, path::PathBuf};
    fn golden(p: &str) -> Vec<u8> { fs::read(PathBuf::from(env!("CARGO_MANIFEST_DIR")).join("../../tests/golden").join(p)).expect(p) }
    fn sp1(name: &str) -> (i32, Vec<u8>, [[u8; 32]; 2]) {
        let b = golden(&format!("sp1/{name}"));
        let (mut variant, mut raw, mut raw_len, mut pi, mut vh) = (0, vec![0u8; 2048], 0usize, [0u8; 64], [0u8; 32]);
        assert_eq!(unsafe { sys::bn254_sp1_fixture_parse(b.as_ptr(), b.len(), &mut variant, raw.as_mut_ptr(), raw.len(), &mut raw_len, pi.as_mut_ptr(), vh.as_mut_ptr()) }, 0);
        raw.truncate(raw_len);
        let mut inputs = [[0u8; 32]; 2];
        inputs[0].copy_from_slice(&pi[..32]); inputs[1].copy_from_slice(&pi[32..]);
        (variant, raw, inputs)
    }
    /// `test_programs` of the reference (`examples/script/src/main.rs:182-245`), PlonK half: the four fixtures verify against the key recovered from the guest ELF.
    #[test]
    fn reference_plonk_fixtures_verify() {
        let vk = golden("plonk_vk.bin");
        for f in ["fibonacci_plonk_proof.bin", "is-prime_plonk_proof.bin", "sha2_plonk_proof.bin", "tendermint_plonk_proof.bin"] {
            let (variant, proof, inputs) = sp1(f);
            assert_eq!(variant, 2);
            assert_eq!(PlonkVerifier::verify(&proof, &vk, &inputs), Ok(true), "{f}");
            let mut bad = inputs; bad[0][31] ^= 1;
            assert_eq!(PlonkVerifier::verify(&proof, &vk, &bad), Err(PlonkError::OpeningPolyMismatch), "{f}");
        }
    }
    /// A synthetic Groth16 batch from the library's generator: statuses as predicted, `verify` and `verify_batch` agree.
    #[test]
    fn groth16_batch_matches_generator() {
        let (n_public, n) = (2usize, 512usize);
        let mut vk = vec![0u8; unsafe { sys::bn254_synth_groth16_vk_len(n_public) }];
        let (mut proofs, mut inputs, mut expected) = (vec![0u8; 256 * n], vec![0u8; 32 * n_public * n], vec![0u8; n]);
        assert_eq!(unsafe { sys::bn254_synth_groth16(0xB2540000, n_public, n, 8, 1, 0, vk.as_mut_ptr(), proofs.as_mut_ptr(), inputs.as_mut_ptr(), expected.as_mut_ptr()) }, 0);
        let pvk = PreparedGroth16Vk::new(&vk, VkMode::Reference).unwrap();
        assert_eq!(pvk.num_public(), n_public);
        let st = pvk.verify_batch_raw(&proofs, 256, &inputs, n_public, n, 0, 0).unwrap();
        assert!(st.iter().zip(&expected).all(|(s, e)| *s == Status::from(*e)));
        let rlc = pvk.verify_batch_raw(&proofs, 256, &inputs, n_public, n, 0, FLAG_RLC).unwrap();
        assert_eq!(st, rlc);
        let one: Vec<[u8; 32]> = inputs[..64].chunks(32).map(|c| c.try_into().unwrap()).collect();
        assert_eq!(Groth16Verifier::verify(&proofs[..256], &vk, &one), Ok(true));
        assert_eq!(Groth16Verifier::verify(&proofs[..256], &vk, &one[..1]), Err(Groth16Error::PrepareInputsFailed));
        assert_eq!(shard_bounds(1 << 20, 8, 3), (3 << 17, 1 << 17));
    }
}
