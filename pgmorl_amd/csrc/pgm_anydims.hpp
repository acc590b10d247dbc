// The runtime-dim kernel family (pgm_anydims.hip, pgm_ppo_any.hip): its one compiled bucket and its range check.
#pragma once
#include "pgm_dispatch.hpp"

namespace pgm {

// the family is compiled once, for these dims, and launched with the true (o, a, k) <= them
constexpr int OM = 32, AM = 8, KM = 3;

// After NULL pointers and check_dims: the range of the family, then pgm_dims.LN (plain towers only).
// head: 0 Gaussian (1 <= A <= 8 action dims), 1 Categorical (2 <= A <= 8 actions).
inline int check_any_dims(const pgm_dims* d, int head, const char* what) {
    if (d->O > OM) {
        set_error("%s: obs_dim %d > %d: the runtime-dim kernels keep layer 1 in one 32-column tile", what, d->O, OM);
        return PGM_E_UNSUPPORTED;
    }
    if (d->A > AM) {
        set_error("%s: A = %d > %d action dims / actions unsupported by the runtime-dim kernels", what, d->A, AM);
        return PGM_E_UNSUPPORTED;
    }
    if (d->K > KM) {
        set_error("%s: K = %d > %d objectives unsupported by the runtime-dim kernels", what, d->K, KM);
        return PGM_E_UNSUPPORTED;
    }
    if (head != 0 && head != 1) {
        set_error("%s: head = %d (0 Gaussian, 1 Categorical)", what, head);
        return PGM_E_UNSUPPORTED;
    }
    if (head == 1 && d->A < 2) {
        set_error("%s: a Categorical head needs A >= 2 actions (got %d)", what, d->A);
        return PGM_E_UNSUPPORTED;
    }
    if (d->LN != 0) {
        set_error("%s: pgm_dims.LN = %d: LayerNorm towers are not built at runtime dims (LN must be 0)", what, d->LN);
        return PGM_E_UNSUPPORTED;
    }
    return PGM_OK;
}

}  // namespace pgm
