// bn254_capi_pairing_rlc.h -- the constants of BN254_FLAG_RLC on the batch pairing product (bn254_capi_pairing_rlc.hip).  Private like bn254_capi_internal.h.
#pragma once

#define PBR_RLC_MIN_FLOOR 64
// BN254_FLAG_RLC is honoured from this many items per launch on unless bn254_set_pairing_rlc_params / BN254_PAIRING_RLC_MIN say otherwise: the smallest measured size
// at which the flag wins by more than the spread at (2, 0b11) -- 4.44 against 8.89 ms at 16 384 items, 4.43 against 2.33 ms at 4096 (profiles/r20_pairing_rlc.txt).
// It is honoured only for items of at most PBR_MAX_VAR_HONOURED variable positions: (4, 0b1110), (4, 0) and (8, 0) lose at every measured size (1.09 .. 5.57 of the
// exact time; same file), and (1, 0) wins at 65 536 alone, so a shape with a variable position takes the exact path.  The probe bn254_dbg_set_pairing_rlc_max_var
// moves the bound for the tests
#define PBR_RLC_MIN_DEFAULT 16384
#define PBR_MAX_VAR_HONOURED 0
