// Scalarised clipped-PPO update for LayerNorm towers (pgm_dims.LN = 1) on the f32 matrix cores
// (v_mfma_f32_32x32x2_f32, exact fp32): ppo_update_ln_kernel.
//
// Each tower layer is Linear(bias=False) -> LayerNorm(64, elementwise_affine) -> tanh (a2c_ppo_acktr/model.py:201-256
// with layernorm=True).  One 256-thread workgroup per tower, two per task, parameters and Adam moments LDS-resident,
// the squared gradient norm the only coupling inside a step: the work split, the tile layout (samples on accumulator
// registers, features on lanes) and every phase but the ones below are the shared tower functions of
// pgm_ppo_tower.hpp (which ppo_update_cat_kernel is built from as well); the loss terms, clip_grad_norm_ and Adam are
// pgm_ppo_terms.hpp's (a2c_ppo_acktr/algo/ppo.py:58-115).  This file holds what is LayerNorm's own: the image with
// gamma / beta slots, the normalisation tiles handed to the shared tile functions as the activation and its backward,
// the Gaussian actor loss, the logstd slot and the 1 / std^2 refresh after Adam.
//
// In that layout a sample's 64 pre-activations sit in ONE register index of the two column tiles over the 32 lanes of
// a half-wave: the LayerNorm row statistics (mean, variance of the mean-subtracted values; in the backward pass
// mean(g) and mean(g xhat)) are sums over the two tiles and the 32 lanes of the half -- one v_permlane16_swap and
// four DPP row rotations each, no LDS and no cross-wave traffic.  The gamma / beta gradients sum over samples, i.e.
// over registers, per lane, like the bias gradients of the plain kernels.
//
// Forward per layer:  z = x W^T, mu = mean(z), var = mean((z - mu)^2), r = 1/sqrt(var + 1e-5), xhat = (z - mu) r,
//                     y = xhat gamma + beta, h = tanh(y).
// Backward:           dy = dh (1 - h^2), dgamma += dy xhat, dbeta += dy, g = dy gamma,
//                     dz = r (g - mean(g) - xhat mean(g xhat)), then dW^T += x^T dz.
// Rows past the end of a ragged minibatch are zero inputs with zero loss gradients: dy = 0 there, so nothing
// reaches dgamma / dbeta, and 1e-5 keeps r finite at z = 0.
//
// The minibatch rows are gathered straight from the rollout storage through the permutation (no packed table).
#include <stdio.h>
#include <stdlib.h>

#include "pgm_dispatch.hpp"
#include "pgm_ppo_tower.hpp"

PGM_STAMP_UNIT(ln)

namespace pgm {

// One LayerNorm tower as an LDS image (TowerImg with gamma / beta in place of the layer biases)
template <int O, int A, int K>
struct LnImg {
    static constexpr int Q = qmax<A, K>();
    float W1t[O][H];
    float W2t[H][SCR];
    float Wh[Q][H];
    float g1[H], be1[H], g2[H], be2[H], bh[Q], logstd[A];
};
// image slot -> flat parameter index (pgm_param_layout_ln order), -1 for padding / unused slots
template <int O, int A, int K>
__device__ __forceinline__ int ln_img_to_flat(int i, int m, const LayoutLN& L) {
    constexpr int Q = qmax<A, K>();
    constexpr int s1 = O * H, s2 = s1 + H * SCR, s3 = s2 + Q * H, s4 = s3 + 4 * H, s5 = s4 + Q, s6 = s5 + A;
    const int NQ = m == 0 ? K : A;
    const int b = m ? PGM_PL_ACTOR_W1 : PGM_PL_CRITIC_W1;  // W1, g1, be1, W2, g2, be2 consecutive
    if (i < s1) return L.off[b] + i;
    if (i < s2) {
        const int j = i - s1, in = j / SCR, o = j - in * SCR;
        return o < H ? L.off[b + 3] + in * H + o : -1;
    }
    if (i < s3) {  // reference head weight [NQ][H] stored transposed [H][NQ]
        const int j = i - s2, q = j / H, u = j - q * H;
        return q < NQ ? L.off[m ? PGM_PL_MEAN_W : PGM_PL_VALUE_W] + u * NQ + q : -1;
    }
    if (i < s4) {
        const int j = i - s3, v = j / H, u = j - v * H;  // g1, be1, g2, be2
        return L.off[b + (v == 0 ? 1 : v == 1 ? 2 : v == 2 ? 4 : 5)] + u;
    }
    if (i < s5) return (i - s4) < NQ ? L.off[m ? PGM_PL_MEAN_B : PGM_PL_VALUE_B] + (i - s4) : -1;
    if (i < s6) return m ? L.off[PGM_PL_LOGSTD] + (i - s5) : -1;
    return -1;
}

using LnArgs = TowerArgs<LayoutLN>;

// obs | action | old logp | adv | old value | return; the actor's per-sample logstd terms and 1 / std^2 on top
template <int O, int A, int K>
struct LnSmem : TowerSmem<LnImg<O, A, K>, O + A + 2 + 2 * K, qmax<A, K>()> {
    float dls[4][TS][qmax<A, K>()];  // per-wave per-sample dL/d(logstd) of the current tile (actor)
    float aiv[A];                    // actor 1 / std^2 = exp(-2 logstd), refreshed by Adam
};

// sum over the 32 lanes of each half-wave, result in all of them: fold the two 16-lane rows of the half
// (v_permlane16_swap), then four DPP rotations inside the row
__device__ __forceinline__ float half32_sum(float v) { return row_sum16(pl16_fold(v, v)); }
// 1 / sqrt(x): hardware estimate + one Newton step (<= 1 ulp)
__device__ __forceinline__ float rsqrt_nr(float x) {
    const float r = __builtin_amdgcn_rsqf(x);
    return r * fmaf(-0.5f * x * r, r, 1.5f);
}

// LayerNorm + affine + tanh of one tile in C layout: z (two column tiles) -> xhat, rstd per register, h
__device__ __forceinline__ void ln_forward_tile(const f32x16 (&z)[2], f32x16 (&xh)[2], float (&rs)[16],
                                                f32x16 (&hout)[2], const float* g, const float* be, int c) {
    const float g0 = g[c], g1 = g[TS + c], b0 = be[c], b1 = be[TS + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float mu = half32_sum(z[0][r] + z[1][r]) * (1.f / 64.f);
        const float d0 = z[0][r] - mu, d1 = z[1][r] - mu;
        const float var = half32_sum(fmaf(d0, d0, d1 * d1)) * (1.f / 64.f);
        const float rr = rsqrt_nr(var + 1e-5f);
        rs[r] = rr;
        xh[0][r] = d0 * rr;
        xh[1][r] = d1 * rr;
        hout[0][r] = tanh_fast(fmaf(xh[0][r], g0, b0));
        hout[1][r] = tanh_fast(fmaf(xh[1][r], g1, b1));
    }
}
// Backward of the same: dh (two column tiles) -> dz (in place); accumulates the per-lane gamma / beta gradients
__device__ __forceinline__ void ln_backward_tile(f32x16 (&dh)[2], const f32x16 (&hv)[2], const f32x16 (&xh)[2],
                                                 const float (&rs)[16], const float* g, int c, float (&gG)[2],
                                                 float (&gBe)[2]) {
    const float g0 = g[c], g1 = g[TS + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float dy0 = dh[0][r] * fmaf(-hv[0][r], hv[0][r], 1.f);
        const float dy1 = dh[1][r] * fmaf(-hv[1][r], hv[1][r], 1.f);
        gG[0] = fmaf(dy0, xh[0][r], gG[0]);
        gG[1] = fmaf(dy1, xh[1][r], gG[1]);
        gBe[0] += dy0;
        gBe[1] += dy1;
        const float q0 = dy0 * g0, q1 = dy1 * g1;
        const float m1 = half32_sum(q0 + q1) * (1.f / 64.f);
        const float m2 = half32_sum(fmaf(q0, xh[0][r], q1 * xh[1][r])) * (1.f / 64.f);
        dh[0][r] = rs[r] * (q0 - m1 - xh[0][r] * m2);
        dh[1][r] = rs[r] * (q1 - m1 - xh[1][r] * m2);
    }
}

template <int O, int A, int K, bool TASKS>
__global__ __launch_bounds__(MT) void ppo_update_ln_kernel(TaskArgsT<LnArgs, TASKS> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Sm = LnSmem<O, A, K>;
    auto& S = *reinterpret_cast<Sm*>(smem_raw);
    constexpr int Q = qmax<A, K>();
    constexpr int IMG = Sm::IMG, NC = Sm::NC, RW = Sm::RW;
    constexpr int oG1 = O * H + H * SCR + Q * H, oBe1 = oG1 + H, oG2 = oBe1 + H, oBe2 = oG2 + H, oBh = oBe2 + H,
                  oLs = oBh + Q;
    constexpr int cLp = O + A, cAdv = O + A + 1, cV = O + A + 2, cR = O + A + 2 + K;  // columns of a gathered row
    const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    int p, m;
    if (!tower_block(a.P, p, m)) return;
    if constexpr (TASKS) take_task_hparams(a.hp, a.hp_task, p);
    const TowerTask<TaskArgsT<LnArgs, TASKS>> k(a, p, m, O, A, K);
    const int NQ = m == 0 ? K : A;

    auto& W = S.Pm;
    float* Pf = &W.W1t[0][0];
    auto to_flat = [&](int i) { return ln_img_to_flat<O, A, K>(i, m, a.L); };
    if (t < A) S.aiv[t] = expf(-2.f * k.P[a.L.off[PGM_PL_LOGSTD] + t]);
    tower_img_load<IMG>(Pf, S.MV, k, to_flat);
    const float* lstd = W.logstd;  // critic: zeros, unused

    float st_v = 0.f, st_a = 0.f, st_e = 0.f;
    int nstep = 0;
    AdamScalars adam(k.b1, k.b2, k.step0);
    float* scr = &S.big.scr[w][0][0];
    float* rt = &S.rows[w][0][0];
    const float* row = rt + c * RW;  // this lane's sample
    PGM_STAMP_DECL

    for (int e = 0; e < k.E; ++e) {
        for (int bb = 0; bb < k.nb; ++bb) {
            const int32_t* perm = a.perms + (size_t)e * k.B + bb * k.mb;
            TowerGrads<Q> g{};
            float gG1[2] = {0.f, 0.f}, gBe1[2] = {0.f, 0.f}, gG2[2] = {0.f, 0.f}, gBe2[2] = {0.f, 0.f};
            float gls = 0.f;  // lanes 32 + q (actor): logstd gradient q
            float lsum = 0.f;

            for (int tile = w; tile * TS < k.mb; tile += 4) {
                const bool ok = tower_gather_tile<NC, RW>(rt, perm, tile * TS, k.mb, h, c, [&](int idx, int col) {
                    if (col < O) return k.obs[(size_t)idx * O + col];
                    if (col < cLp) return k.actions[(size_t)idx * A + (col - O)];
                    if (col == cLp) return k.logp[idx];
                    if (col == cAdv) return k.adv[idx];
                    if (col < cR) return k.values[(size_t)idx * K + (col - cV)];
                    return k.returns[(size_t)idx * K + (col - cR)];
                });
                PGM_STAMP(0);
                f32x16 X1[2], H1[2], X2[2], H2[2];  // xhat and tanh output of the two layers
                float rs1[16], rs2[16], outv[Q];
                tower_forward_tile<O, Q, RW>(
                    rt, scr, W, h, c, H1, H2, outv,
                    [&](const f32x16(&z)[2], f32x16(&ho)[2]) { ln_forward_tile(z, X1, rs1, ho, W.g1, W.be1, c); },
                    [&](const f32x16(&z)[2], f32x16(&ho)[2]) { ln_forward_tile(z, X2, rs2, ho, W.g2, W.be2, c); });
                PGM_STAMP(16);
                // ---- per-sample loss gradients (ppo.py:80-96); both halves compute the same sample
                float dO[Q] = {};
                if (m == 0) {  // value loss
                    const float ls = tower_value_loss<K>(dO, outv, row + cV, row + cR, k.clip,
                                                         a.hp.use_clipped_value_loss, ok, k.vscale);
                    if (ok && h == 0) lsum += ls;
                } else {  // diagonal Gaussian log-prob, clipped surrogate
                    float lp = 0.f;
#pragma unroll
                    for (int q = 0; q < A; ++q) {
                        const float diff = row[O + q] - outv[q];
                        lp += -0.5f * diff * diff * S.aiv[q] - lstd[q] - LOG_SQRT_2PI;
                    }
                    const float ratio = expf(lp - row[cLp]);
                    const LossTerm sg = surrogate_term(ratio, row[cAdv], k.clip);
                    const float dlp = ok ? k.ascale * sg.grad * ratio : 0.f;
                    if (ok && h == 0) lsum += sg.loss;
#pragma unroll
                    for (int q = 0; q < A; ++q) {
                        const float diff = row[O + q] - outv[q];
                        const float iv = S.aiv[q];
                        dO[q] = dlp * diff * iv;
                        if (h == 0) S.dls[w][c][q] = dlp * (diff * diff * iv - 1.f);
                    }
                }
                PGM_STAMP(17);
                tower_backward_tile<O, Q, RW>(
                    g, dO, &S.dout[w][0][0], rt, scr, W, H1, H2, h, c,
                    [&](f32x16(&z)[2], const f32x16(&hv)[2]) { ln_backward_tile(z, hv, X2, rs2, W.g2, c, gG2, gBe2); },
                    [&](f32x16(&z)[2], const f32x16(&hv)[2]) { ln_backward_tile(z, hv, X1, rs1, W.g1, c, gG1, gBe1); });
                if (h == 1 && m == 1 && c < A) tile_col_add<Q>(gls, &S.dls[w][0][0] + c);
                PGM_STAMP(7);
            }  // tiles

            // ---- combine the lane halves of the per-column partial sums
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                gG1[i] = half_sum(gG1[i]);
                gBe1[i] = half_sum(gBe1[i]);
                gG2[i] = half_sum(gG2[i]);
                gBe2[i] = half_sum(gBe2[i]);
            }
            lsum = wave_sum64(lsum);
            if (l == 0) S.red[8 + w] = lsum;
            lds_sync_m();  // every wave's tiles done: the gradient image overwrites the transpose tiles
            PGM_STAMP(12);
            tower_reduce_image<O, Q>(
                S.big.G, g, NQ, oBh,
                [&](auto acc, int i) {
                    acc(oG1 + i * TS + c, gG1[i]);
                    acc(oBe1 + i * TS + c, gBe1[i]);
                    acc(oG2 + i * TS + c, gG2[i]);
                    acc(oBe2 + i * TS + c, gBe2[i]);
                },
                [&](auto acc, bool add) {  // -entropy_coef * d(mean entropy)/d logstd enters once (ppo.py:98)
                    if (h == 1 && c < A) acc(oLs + c, m == 1 ? gls - (add ? 0.f : a.hp.entropy_coef) : 0.f);
                });
            PGM_STAMP(2);
            if (t == 0) {
                const float ls = sum4(S.red + 8);
                if (m == 0) st_v += ls * k.vstat;
                else st_a += ls * k.astat;
                float ent = 0.f;  // entropy with the logstd of this step (before Adam)
#pragma unroll
                for (int q = 0; q < A; ++q) ent += 0.5f + LOG_SQRT_2PI + lstd[q];
                st_e += ent;
            }
            tower_clip_adam<IMG>(S.big.G, S.MV, Pf, S.red, a, k, nstep, adam, [&](int i, float pp) {
                if (m == 1 && i >= oLs && i < oLs + A) S.aiv[i - oLs] = expf(-2.f * pp);
            });
            PGM_STAMP(3);
        }  // minibatches
    }      // epochs
    tower_img_store<IMG>(Pf, S.MV, k, to_flat);
    if (t == 0) tower_write_stats(a, k, nstep, st_v, st_a, st_e);
    PGM_STAMP_FLUSH;
}

int describe_update_ln(char* buf, int n) {
    return snprintf(buf, n, "ppo_update_ln_kernel (one workgroup per tower)");
}

int ppo_update_ln(const pgm_dims* d, const pgm_ppo_hparams* hp, float* params, float* adam_m, float* adam_v,
                  int32_t* adam_step, const float* lr, const int32_t* perms, const pgm_rollout_buf* rb, float* stats,
                  void* workspace, hipStream_t stream, const pgm_task_hparams* hp_task) {
    if (!workspace) {
        set_error("pgm_ppo_update: the LayerNorm update needs the workspace (pgm_ppo_update_workspace_bytes)");
        return PGM_E_INVALID_ARG;
    }
    LnArgs a{d->P, d->N, d->T, make_layout_ln(d->O, d->A, d->K, d->H), *hp, params, adam_m, adam_v, adam_step, lr,
             perms, rb->obs, rb->actions, rb->logp, rb->values, rb->returns, rb->adv, stats,
             (unsigned long long*)workspace, dbg_delay_hook()};
    return dispatch_dims(d->O, d->A, d->K, "pgm_ppo_update", [&](auto o, auto aa, auto k) -> int {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        if constexpr (O > 32) {
            set_error("pgm_ppo_update: LayerNorm towers need obs_dim <= 32 (got %d)", O);
            return PGM_E_UNSUPPORTED;
        } else {
            const char* need = "pgm_ppo_update: the LayerNorm update runs one workgroup per tower and needs 2 P = %d "
                               "<= %d CUs; shard the tasks over more GPUs";
            if (hp_task)
                return launch_tower_update<sizeof(LnSmem<O, A, K>)>(
                    ppo_update_ln_kernel<O, A, K, true>, with_task_table(a, hp_task), stream, "pgm_ppo_update", need);
            return launch_tower_update<sizeof(LnSmem<O, A, K>)>(ppo_update_ln_kernel<O, A, K, false>, a, stream,
                                                                "pgm_ppo_update", need);
        }
    });
}

}  // namespace pgm
