"""MI355X-native batch BN254 verifier: Python-side access to the C ABI (include/bn254_verify.h).

The product is the shared library built from csrc/ (HIP kernels + C ABI); this package only loads it with ctypes so that
tests, __graft_entry__ and bench.py can call the same entry points a Rust/C host would bind.  There is no Python or CPU
implementation of verification here: if the library or a GPU is missing, calls raise.
"""
from .binding import (  # noqa: F401
    ACCEPT, REJECT, ERR_NOT_MEMBER, ERR_NOT_ON_CURVE, ERR_NOT_IN_SUBGROUP, ERR_INPUT_LEN, ERR_MALFORMED,
    VK_REFERENCE, VK_GNARK, Bn254Error, Groth16Verifier, PreparedVk, build, lib, lib_path, synth_groth16, kernel_kinds,
    set_profile_kernels, PreparedPlonkVk, PlonkVerifier, FLAG_STRICT_SCALARS, FLAG_RLC, RAW_PROOF_LEN, proof_write_raw, shard_plan, set_rlc_params, set_plonk_params,
    dbg_rlc_wide_group, dbg_rlc_wide_plan, dbg_rlc_groups, FLAG_COMPRESSED_PROOFS, COMPRESSED_PROOF_LEN, compress_proof, dbg_g16_decompress,
    sp1_public_values_digest, sp1_pack_values, dbg_sp1_public_inputs, synth_groth16_for_inputs, KeySet, dbg_keys_group,
    set_keys_params, dbg_keys_plan, prepare_vks, dbg_prepare_vks, dbg_pvk_image, VK_PREPARE_STAGES, synth_plonk, synth_plonk_for_inputs, dbg_plonk_stages, dbg_plonk_stages_keys,
    PlonkKeySet, dbg_plonk_keys_plan, last_diagnostic, set_plonk_keys_params, set_plonk_rlc_params, dbg_plonk_keys_knobs,
    device_selftest, selftest_state, selftest_check_names, dbg_selftest, Bn254SelfTestError, E_SELFTEST, dbg_overlap_replay,
    pairing_check_batch, pairing_batch, pairing_check_batch_device, pairing_reserve, dbg_pairing_batch, dbg_pairing_plan, PAIRING_MAX_PAIRS, PAIRING_PAIR_LEN,
    set_pairing_params, pairing_params, pairing_state, set_pairing_rlc_params, pairing_rlc_params, pairing_rlc_state, dbg_pairing_batch_rlc, dbg_set_pairing_rlc_max_var, dbg_pairing_form, PAIRING_FORM_LANES, PAIRING_FORM_COOP,
    g2_prepare, pairing_check_batch_shared, pairing_batch_shared, pairing_check_batch_shared_device, dbg_pairing_batch_shared, pairing_packed_len, G2_PREPARED_LEN,
    PAIRING_G1_LEN,
    kzg_key_prepare, kzg_verify_batch, kzg_verify_batch_device, kzg_reserve, set_kzg_params, kzg_params, kzg_state, dbg_kzg_fold, KZG_OPENING_LEN, KZG_KEY_LEN,
    kzg_verify_folded_batch, kzg_verify_folded_batch_device, kzg_fold_reserve, dbg_kzg_fold_proof, dbg_kzg_fold_plan, kzg_fold_len, KZG_FOLD_MAX_DIGESTS, KZG_FOLD_MAX_DATA,
    g1_bases_prepare, G1Bases, g1_msm_batch, g1_msm_batch_device, g1_msm_reserve, g1_msm_item_len, dbg_g1_msm_batch, dbg_g1_msm_batch_plan, dbg_g1_msm_batch_state,
    G1_MSM_MAX_VAR, G1_MSM_MAX_UNIT, G1_MSM_MAX_SHARED,
    dbg_g16_loader, dbg_g16_loader_keys, G16_LOADER_LANES, G16_LOADER_COMPACT, G16_LOADER_WIDE, G16_LOADER_WIDE8, G16_LOADER_POINTS_LEN,
)
