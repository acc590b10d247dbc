// The arithmetic every PPO update kernel shares, in one place: the per-sample loss terms with their tie semantics
// (a2c_ppo_acktr/algo/ppo.py:76-103), clip_grad_norm_'s coefficient, the Adam element step and its per-step scalars,
// and the bounded poll / two-tower norm hand-off of the tagged 8-byte granules.
//
// The loss terms are plain C++: a host compiler builds them without HIP (tests/native/ppo_terms_shim.cpp), so the tie
// weights are tested against torch autograd off the GPU.  Everything below the __HIPCC__ guard is device code.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include "pgm_common.hpp"
#define PGM_HD __host__ __device__ __forceinline__
#else
#define PGM_HD inline
#endif

namespace pgm {

// torch.min(a,b) / torch.max(a,b) backward weights for the first argument (ties split the gradient in half)
PGM_HD float wmin2(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
PGM_HD float wmax2(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

struct LossTerm {
    float grad;  // d(term) / d(first argument), before the caller's batch scale
    float loss;
};

// Value loss of one output without its 0.5 (the callers' scales carry it): clipped, max((V - R)^2, (vc - R)^2) with
// vc = Vold + clamp(V - Vold, -clip, clip); the clamp passes its gradient on the closed interval and torch.max splits
// a tie in half.  Unclipped, (R - V)^2.  grad is d loss / d V.
PGM_HD LossTerm value_loss_term(float V, float Vold, float R, float clip, bool clipped) {
    if (clipped) {
        const float dv = V - Vold;
        const float vc = Vold + fminf(fmaxf(dv, -clip), clip);
        const float l1 = (V - R) * (V - R), l2 = (vc - R) * (vc - R);
        const float inr = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
        return {wmax2(l1, l2) * 2.f * (V - R) + wmax2(l2, l1) * 2.f * (vc - R) * inr, fmaxf(l1, l2)};
    }
    return {2.f * (V - R), (R - V) * (R - V)};
}

// Clipped surrogate: s1 = ratio adv, s2 = clamp(ratio, 1 - clip, 1 + clip) adv; torch.min splits a tie in half and
// the clamp passes its gradient on the closed interval.  grad is d min(s1, s2) / d ratio (the callers' -1 / mb scale
// turns it into the loss gradient), loss is -min(s1, s2).
PGM_HD LossTerm surrogate_term(float ratio, float adv, float clip) {
    const float s1 = ratio * adv;
    const float s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * adv;
    const float inr = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? 1.f : 0.f;
    return {adv * (wmin2(s1, s2) + wmin2(s2, s1) * inr), -fminf(s1, s2)};
}

#ifdef __HIPCC__
// clip_grad_norm_'s coefficient min(max_norm / (sqrt(sum of squares) + 1e-6), 1) (torch nn/utils/clip_grad.py):
// hardware sqrt and a Newton-refined reciprocal (<= 1 ulp) instead of the IEEE expansions, off the critical path's
// division sequences
__device__ __forceinline__ float clip_coef(float max_norm, float sumsq) {
    const float d = __builtin_amdgcn_sqrtf(sumsq) + 1e-6f;
    float r = __builtin_amdgcn_rcpf(d);
    r = fmaf(fmaf(-d, r, 1.f), r, r);
    return fminf(max_norm * r, 1.f);
}

// torch Adam on one element with the clipped gradient g * coef: p -= step_size * m / (sqrt(v) / sqrt(bc2) + eps), on
// the hardware sqrt / rcp (<= 2 ulp on the step)
__device__ __forceinline__ void adam_step(float g, float coef, float& m, float& v, float& p, float b1, float b2,
                                          float step_size, float inv_bc2s, float eps) {
    const float gc = g * coef;
    m = m + (1.f - b1) * (gc - m);
    v = v * b2 + (1.f - b2) * (gc * gc);
    const float den = __builtin_amdgcn_sqrtf(v) * inv_bc2s + eps;
    p -= step_size * m * __builtin_amdgcn_rcpf(den);
}

// beta1^step and beta2^step in fp64, advanced once per Adam step to the two fp32 scalars of adam_step
struct AdamScalars {
    double b1p, b2p;
    float step_size, inv_bc2s;
    __device__ __forceinline__ AdamScalars(float b1, float b2, int step0)
        : b1p(pow((double)b1, (double)step0)), b2p(pow((double)b2, (double)step0)), step_size(0.f), inv_bc2s(0.f) {}
    __device__ __forceinline__ void advance(double lr, float b1, float b2) {
        b1p = b1p * (double)b1;
        b2p = b2p * (double)b2;
        step_size = (float)(lr / (1.0 - b1p));
        inv_bc2s = 1.f / (float)sqrt(1.0 - b2p);
    }
};

// Bounded spin on a tagged 8-byte granule (tag in the high word): the granule once its tag matches; after 2^26 polls
// fail_value is stored to the launch's fail word and 0 returned.
__device__ __forceinline__ unsigned long long poll_tagged(const unsigned long long* granule, unsigned tag,
                                                          unsigned long long* fail_word,
                                                          unsigned long long fail_value) {
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long x = __hip_atomic_load(granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(x >> 32) == tag) return x;
        if (spins > (1u << 26)) {  // the writer never arrived: flag the launch as failed
            __hip_atomic_store(fail_word, fail_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return 0;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Two-tower hand-off of the squared gradient norm, by one lane of tower m's workgroup: ws_pair holds the critic's and
// the actor's granule of this step parity.  Publishes `total` under `tag`, waits for the partner's (not at all once
// the launch is flagged as failed) and returns critic + actor, the same bits in both workgroups.
__device__ __forceinline__ float tower_norm_exchange(unsigned long long* ws_pair, int m, unsigned tag, float total,
                                                     unsigned long long* fail_word, const DbgDelay& dbg, int nstep) {
    __hip_atomic_store(ws_pair + m, ((unsigned long long)tag << 32) | __float_as_uint(total), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    dbg_delay(dbg, nstep, 2);
    const bool failed = __hip_atomic_load(fail_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long x = failed ? 0ull : poll_tagged(ws_pair + (1 - m), tag, fail_word, 1ull);
    const float other = __uint_as_float((unsigned)x);
    return m == 0 ? total + other : other + total;
}
#endif  // __HIPCC__

}  // namespace pgm
