// Compile-time (obs, action, objective) dims of the supported SynthMO envs.
#pragma once
#include <type_traits>

#include "pgm_common.hpp"

namespace pgm {

template <int V>
using ic = std::integral_constant<int, V>;

// (O, A, K): Walker2d/HalfCheetah, Hopper-v2, Hopper-v3, Humanoid, Ant, Swimmer (SURVEY.md §8 header table), then the
// native MO-Dummy-v0 / MO-Dummy3-v0 (pgm_dummy.hpp).
// f(ic<O>, ic<A>, ic<K>) -> int status.
template <class F>
int dispatch_dims(int O, int A, int K, const char* what, F&& f) {
    if (O == 17 && A == 6 && K == 2) return f(ic<17>{}, ic<6>{}, ic<2>{});
    if (O == 11 && A == 3 && K == 2) return f(ic<11>{}, ic<3>{}, ic<2>{});
    if (O == 11 && A == 3 && K == 3) return f(ic<11>{}, ic<3>{}, ic<3>{});
    if (O == 376 && A == 17 && K == 2) return f(ic<376>{}, ic<17>{}, ic<2>{});
    if (O == 27 && A == 8 && K == 2) return f(ic<27>{}, ic<8>{}, ic<2>{});
    if (O == 8 && A == 2 && K == 2) return f(ic<8>{}, ic<2>{}, ic<2>{});
    if (O == 6 && A == 2 && K == 2) return f(ic<6>{}, ic<2>{}, ic<2>{});
    if (O == 6 && A == 2 && K == 3) return f(ic<6>{}, ic<2>{}, ic<3>{});
    set_error("%s: unsupported dims O=%d A=%d K=%d (supported: 17/6/2, 11/3/2, 11/3/3, 376/17/2, 27/8/2, 8/2/2, 6/2/2, "
              "6/2/3)", what, O, A, K);
    return PGM_E_UNSUPPORTED;
}

// (O, A, K) of the discrete-action envs (Categorical head; A = number of actions): Deep Sea Treasure.  One X(...) per
// dim set; the *_cat entry points and pgm_env_ingest instantiate their kernels for each.
#define PGM_CAT_DIMS(X) X(3, 4, 2)
inline bool is_cat_dims(int O, int A, int K) {
#define PGM_X(o, a, k) if (O == o && A == a && K == k) return true;
    PGM_CAT_DIMS(PGM_X)
#undef PGM_X
    return false;
}
template <class F>
int dispatch_dims_cat(int O, int A, int K, const char* what, F&& f) {
#define PGM_X(o, a, k) if (O == o && A == a && K == k) return f(ic<o>{}, ic<a>{}, ic<k>{});
    PGM_CAT_DIMS(PGM_X)
#undef PGM_X
#define PGM_STR_(x) #x
#define PGM_X(o, a, k) " " PGM_STR_(o) "/" PGM_STR_(a) "/" PGM_STR_(k)
    set_error("%s: unsupported dims O=%d A=%d K=%d for a Categorical head (supported, A = number of actions:" PGM_CAT_DIMS(
                  PGM_X) ")", what, O, A, K);
#undef PGM_X
#undef PGM_STR_
    return PGM_E_UNSUPPORTED;
}

inline int check_dims(const pgm_dims* d, const char* what) {
    if (!d) {
        set_error("%s: null dims", what);
        return PGM_E_INVALID_ARG;
    }
    if (d->P <= 0 || d->N <= 0 || d->T < 0 || d->O <= 0 || d->A <= 0 || d->K <= 0) {
        set_error("%s: non-positive dims P=%d N=%d T=%d O=%d A=%d K=%d", what, d->P, d->N, d->T, d->O, d->A, d->K);
        return PGM_E_SHAPE;
    }
    if (d->H != H) {
        set_error("%s: hidden size %d unsupported (this build is H=%d, model.py:202)", what, d->H, H);
        return PGM_E_UNSUPPORTED;
    }
    if (d->N > 8) {
        set_error("%s: N=%d envs per task > 8 unsupported", what, d->N);
        return PGM_E_UNSUPPORTED;
    }
    return PGM_OK;
}

// pgm_dims.LN of the entry points that touch the policy: 0 or 1, and LayerNorm towers only where layer 1 is
// LDS-resident (obs_dim <= 32; Humanoid's streamed layer 1 has no LayerNorm kernel)
inline int check_ln(const pgm_dims* d, const char* what) {
    if (d->LN != 0 && d->LN != 1) {
        set_error("%s: pgm_dims.LN = %d (0 plain towers, 1 LayerNorm towers)", what, d->LN);
        return PGM_E_INVALID_ARG;
    }
    if (d->LN == 1 && d->O > 32) {
        set_error("%s: LayerNorm towers are built for obs_dim <= 32 (17/6/2, 11/3/2, 11/3/3, 27/8/2, 8/2/2, 6/2/2, 6/2/3); obs_dim "
                  "%d "
                  "(MO-Humanoid) needs a streamed layer-1 LayerNorm kernel that does not exist", what, d->O);
        return PGM_E_UNSUPPORTED;
    }
    return PGM_OK;
}

// Categorical entry points, after check_dims: the dim set ...
inline int check_cat_dims(const pgm_dims* d, const char* what) {
    return dispatch_dims_cat(d->O, d->A, d->K, what, [](auto, auto, auto) { return (int)PGM_OK; });
}
// ... and, last, pgm_dims.LN: no LayerNorm kernel has a Categorical head
inline int check_cat_ln(const pgm_dims* d, const char* what) {
    if (d->LN != 0) {
        set_error("%s: pgm_dims.LN = %d: LayerNorm towers with a Categorical head are not built (LN must be 0)", what,
                  d->LN);
        return d->LN == 1 ? PGM_E_UNSUPPORTED : PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

}  // namespace pgm
