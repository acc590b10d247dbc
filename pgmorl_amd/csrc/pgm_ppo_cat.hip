// Scalarised clipped-PPO update for discrete-action policies (Categorical head) on the f32 matrix cores
// (v_mfma_f32_32x32x2_f32, exact fp32): ppo_update_cat_kernel.
//
// The towers are the plain ones (Linear -> tanh, twice; a2c_ppo_acktr/model.py:201-256); the head is the reference's
// Categorical (a2c_ppo_acktr/distributions.py:17-27,54-68): logits z = Linear(actor features), one integer action per
// sample.  One 256-thread workgroup per tower, two per task, parameters and Adam moments LDS-resident, the squared
// gradient norm the only coupling inside a step: the work split, the tile layout and every phase but the ones below
// are the shared tower functions of pgm_ppo_tower.hpp (which ppo_update_ln_kernel is built from as well); the value
// loss, the surrogate's tie weights, clip_grad_norm_ and Adam are pgm_ppo_terms.hpp's
// (a2c_ppo_acktr/algo/ppo.py:58-115).  This file holds what is the Categorical head's own: the image without a logstd
// slot, the row columns (one action index), tanh_bias_pk / dtanh_pk as the activation, the actor loss and the entropy
// statistics.  With A = 4 actions the head is VALU work on four columns.
//
// Actor head, per sample i with taken action a (the index stored as fp32 in the width-1 action column):
//     p = softmax(z) (max-subtracted), logp = log p_a, H_i = -sum_j p_j log p_j,
//     ratio = exp(logp - old logp), the clipped surrogate (surrogate_term),
//     dL/dz_j = g_i (1[j = a] - p_j) + (entropy_coef / mb) p_j (log p_j + H_i),
// g_i = dL/dlogp of the surrogate (0 on the clipped branch); the second term is -entropy_coef d(mean H)/dz_j.
// Rows past the end of a ragged minibatch are zero inputs with zero loss gradient and zero entropy.
// The minibatch rows are gathered straight from the rollout storage through the permutation (no packed table).
#include <stdio.h>
#include <stdlib.h>

#include "pgm_dispatch.hpp"
#include "pgm_ppo_tower.hpp"

PGM_STAMP_UNIT(cat)

namespace pgm {

// One tower as an LDS image (TowerImg without the logstd slot)
template <int O, int A, int K>
struct CatImg {
    static constexpr int Q = qmax<A, K>();
    float W1t[O][H];
    float W2t[H][SCR];
    float Wh[Q][H];
    float b1[H], b2[H], bh[Q];
};
// image slot -> flat parameter index (pgm_param_layout_cat order), -1 for padding / unused slots
template <int O, int A, int K>
__device__ __forceinline__ int cat_img_to_flat(int i, int m, const LayoutCat& L) {
    constexpr int Q = qmax<A, K>();
    constexpr int s1 = O * H, s2 = s1 + H * SCR, s3 = s2 + Q * H, s4 = s3 + H, s5 = s4 + H, s6 = s5 + Q;
    const int NQ = m == 0 ? K : A;
    if (i < s1) return L.off[m ? PGM_P_ACTOR_W1 : PGM_P_CRITIC_W1] + i;
    if (i < s2) {
        const int j = i - s1, in = j / SCR, o = j - in * SCR;
        return o < H ? L.off[m ? PGM_P_ACTOR_W2 : PGM_P_CRITIC_W2] + in * H + o : -1;
    }
    if (i < s3) {  // reference head weight [NQ][H] stored transposed [H][NQ]
        const int j = i - s2, q = j / H, u = j - q * H;
        return q < NQ ? L.off[m ? PGM_PC_LINEAR_W : PGM_P_VALUE_W] + u * NQ + q : -1;
    }
    if (i < s4) return L.off[m ? PGM_P_ACTOR_B1 : PGM_P_CRITIC_B1] + (i - s3);
    if (i < s5) return L.off[m ? PGM_P_ACTOR_B2 : PGM_P_CRITIC_B2] + (i - s4);
    if (i < s6) return (i - s5) < NQ ? L.off[m ? PGM_PC_LINEAR_B : PGM_P_VALUE_B] + (i - s5) : -1;
    return -1;
}

using CatArgs = TowerArgs<LayoutCat>;

// obs | action index | old logp | adv | old value | return
template <int O, int A, int K>
using CatSmem = TowerSmem<CatImg<O, A, K>, O + 1 + 2 + 2 * K, qmax<A, K>()>;

template <int O, int A, int K>
__global__ __launch_bounds__(MT) void ppo_update_cat_kernel(CatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Sm = CatSmem<O, A, K>;
    auto& S = *reinterpret_cast<Sm*>(smem_raw);
    constexpr int Q = qmax<A, K>();
    constexpr int IMG = Sm::IMG, NC = Sm::NC, RW = Sm::RW;
    constexpr int oB1 = O * H + H * SCR + Q * H, oB2 = oB1 + H, oBh = oB2 + H;
    constexpr int cA = O, cLp = O + 1, cAdv = O + 2, cV = O + 3, cR = O + 3 + K;  // columns of a gathered row
    const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    int p, m;
    if (!tower_block(a.P, p, m)) return;
    const TowerTask<CatArgs> k(a, p, m, O, 1, K);  // one stored float per action: its index
    const int NQ = m == 0 ? K : A;
    const float escale = a.hp.entropy_coef / (float)k.mb;

    auto& W = S.Pm;
    float* Pf = &W.W1t[0][0];
    auto to_flat = [&](int i) { return cat_img_to_flat<O, A, K>(i, m, a.L); };
    tower_img_load<IMG>(Pf, S.MV, k, to_flat);

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
            float gB1[2] = {0.f, 0.f}, gB2[2] = {0.f, 0.f};
            float lsum = 0.f, esum = 0.f;  // loss and entropy sums of this wave's samples

            for (int tile = w; tile * TS < k.mb; tile += 4) {
                const bool ok = tower_gather_tile<NC, RW>(rt, perm, tile * TS, k.mb, h, c, [&](int idx, int col) {
                    if (col < O) return k.obs[(size_t)idx * O + col];
                    if (col == cA) return k.actions[idx];
                    if (col == cLp) return k.logp[idx];
                    if (col == cAdv) return k.adv[idx];
                    if (col < cR) return k.values[(size_t)idx * K + (col - cV)];
                    return k.returns[(size_t)idx * K + (col - cR)];
                });
                PGM_STAMP(0);
                f32x16 H1[2], H2[2];
                float outv[Q];
                tower_forward_tile<O, Q, RW>(
                    rt, scr, W, h, c, H1, H2, outv,
                    [&](const f32x16(&z)[2], f32x16(&ho)[2]) {
#pragma unroll
                        for (int b = 0; b < 2; ++b) tanh_bias_pk<16>(z[b], W.b1[b * TS + c], ho[b]);
                    },
                    [&](const f32x16(&z)[2], f32x16(&ho)[2]) {
#pragma unroll
                        for (int b = 0; b < 2; ++b) tanh_bias_pk<16>(z[b], W.b2[b * TS + c], ho[b]);
                    });
                PGM_STAMP(16);
                // ---- per-sample loss gradients (ppo.py:80-96); both halves compute the same sample
                float dO[Q] = {};
                if (m == 0) {  // value loss
                    const float ls = tower_value_loss<K>(dO, outv, row + cV, row + cR, k.clip,
                                                         a.hp.use_clipped_value_loss, ok, k.vscale);
                    if (ok && h == 0) lsum += ls;
                } else {  // Categorical log-prob / entropy, clipped surrogate
                    float zm = outv[0];
#pragma unroll
                    for (int q = 1; q < A; ++q) zm = fmaxf(zm, outv[q]);
                    float ex[A], se = 0.f;
#pragma unroll
                    for (int q = 0; q < A; ++q) {
                        ex[q] = expf(outv[q] - zm);
                        se += ex[q];
                    }
                    const float lse = zm + logf(se), rse = 1.f / se;
                    const int ai = (int)row[cA];  // the taken action (exact integer in fp32)
                    float pj[A], lpj[A], lp = outv[0] - lse, ent = 0.f;
#pragma unroll
                    for (int q = 0; q < A; ++q) {
                        pj[q] = ex[q] * rse;
                        lpj[q] = outv[q] - lse;
                        ent = fmaf(-pj[q], lpj[q], ent);
                        lp = ai == q ? lpj[q] : lp;
                    }
                    const float ratio = expf(lp - row[cLp]);
                    const LossTerm sg = surrogate_term(ratio, row[cAdv], k.clip);
                    const float dlp = ok ? k.ascale * sg.grad * ratio : 0.f;
                    const float es = ok ? escale : 0.f;
                    if (ok && h == 0) {
                        lsum += sg.loss;
                        esum += ent;
                    }
#pragma unroll
                    for (int q = 0; q < A; ++q)
                        dO[q] = dlp * ((ai == q ? 1.f : 0.f) - pj[q]) + es * pj[q] * (lpj[q] + ent);
                }
                PGM_STAMP(17);
                // dZ = dH (1 - H^2) in place; the bias gradient sums it over the samples (registers), per lane
                auto dtanh = [&](f32x16(&z)[2], const f32x16(&hv)[2], float(&gB)[2]) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        dtanh_pk<16>(z[b], hv[b], z[b]);
#pragma unroll
                        for (int r = 0; r < 16; ++r) gB[b] += z[b][r];
                    }
                };
                tower_backward_tile<O, Q, RW>(
                    g, dO, &S.dout[w][0][0], rt, scr, W, H1, H2, h, c,
                    [&](f32x16(&z)[2], const f32x16(&hv)[2]) { dtanh(z, hv, gB2); },
                    [&](f32x16(&z)[2], const f32x16(&hv)[2]) { dtanh(z, hv, gB1); });
                PGM_STAMP(7);
            }  // tiles

            // ---- combine the lane halves of the per-column partial sums
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                gB1[i] = half_sum(gB1[i]);
                gB2[i] = half_sum(gB2[i]);
            }
            lsum = wave_sum64(lsum);
            esum = wave_sum64(esum);
            if (l == 0) {
                S.red[8 + w] = lsum;
                S.red[12 + w] = esum;
            }
            lds_sync_m();  // every wave's tiles done: the gradient image overwrites the transpose tiles
            PGM_STAMP(12);
            tower_reduce_image<O, Q>(
                S.big.G, g, NQ, oBh,
                [&](auto acc, int i) {
                    acc(oB1 + i * TS + c, gB1[i]);
                    acc(oB2 + i * TS + c, gB2[i]);
                },
                [](auto, bool) {});
            PGM_STAMP(2);
            if (t == 0) {
                const float ls = sum4(S.red + 8);
                if (m == 0) {
                    st_v += ls * k.vstat;
                } else {
                    st_a += ls * k.astat;
                    st_e += sum4(S.red + 12) * k.astat;
                }
            }
            tower_clip_adam<IMG>(S.big.G, S.MV, Pf, S.red, a, k, nstep, adam, [](int, float) {});
            PGM_STAMP(3);
        }  // minibatches
    }      // epochs
    tower_img_store<IMG>(Pf, S.MV, k, to_flat);
    if (t == 0) tower_write_stats(a, k, nstep, st_v, st_a, st_e);
    PGM_STAMP_FLUSH;
}

}  // namespace pgm

using namespace pgm;

extern "C" {

size_t pgm_ppo_update_cat_workspace_bytes(const pgm_dims* d) { return d && d->P > 0 ? ppo_flag_bytes(d->P) : 0; }

// Validated before any device work: NULL pointers, check_dims, the dim set, the minibatch shape, LN.
int pgm_ppo_update_cat(const pgm_dims* d, const pgm_ppo_hparams* hp, float* params, float* adam_m, float* adam_v,
                       int32_t* adam_step, const float* lr, const int32_t* perms, const pgm_rollout_buf* rb,
                       float* stats, void* workspace, pgm_stream_t stream) {
    if (!d || !hp || !params || !adam_m || !adam_v || !adam_step || !lr || !perms || !rb || !rb->obs || !rb->actions ||
        !rb->logp || !rb->values || !rb->returns || !rb->adv || !stats || !workspace) {
        set_error("pgm_ppo_update_cat: null pointer (the workspace of pgm_ppo_update_cat_workspace_bytes is required)");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_ppo_update_cat")) return rc;
    if (int rc = check_cat_dims(d, "pgm_ppo_update_cat")) return rc;
    if (d->T < 1 || hp->ppo_epoch < 1 || hp->num_mini_batch < 1 || hp->num_mini_batch > d->T * d->N) {
        set_error("pgm_ppo_update_cat: bad shape T=%d N=%d ppo_epoch=%d num_mini_batch=%d", d->T, d->N, hp->ppo_epoch,
                  hp->num_mini_batch);
        return PGM_E_SHAPE;
    }
    if (int rc = check_cat_ln(d, "pgm_ppo_update_cat")) return rc;
    CatArgs a{d->P, d->N, d->T, make_layout_cat(d->O, d->A, d->K, d->H), *hp, params, adam_m, adam_v, adam_step, lr,
              perms, rb->obs, rb->actions, rb->logp, rb->values, rb->returns, rb->adv, stats,
              (unsigned long long*)workspace, dbg_delay_hook()};
    return dispatch_dims_cat(d->O, d->A, d->K, "pgm_ppo_update_cat", [&](auto o, auto aa, auto k) -> int {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        static_assert(O <= 32, "ppo_update_cat_kernel keeps layer 1 LDS-resident (one input tile)");
        return launch_tower_update<sizeof(CatSmem<O, A, K>)>(
            ppo_update_cat_kernel<O, A, K>, a, (hipStream_t)stream, "pgm_ppo_update_cat",
            "pgm_ppo_update_cat: the update runs one workgroup per tower and needs 2 P = %d <= %d CUs; "
            "shard the tasks over more GPUs");
    });
}

}  // extern "C"
