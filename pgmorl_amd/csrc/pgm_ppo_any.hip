// Scalarised clipped-PPO update at runtime dims (pgm_abi_feature_mask() & PGM_FEATURE_ANY_DIMS):
// ppo_update_any_kernel.
//
// Plain towers (Linear -> tanh, twice; a2c_ppo_acktr/model.py:201-256) with a Gaussian or a Categorical head, compiled
// once for (OM, AM, KM) = (32, 8, 3) and launched with the true dims (o, a, k).  One 256-thread workgroup per tower,
// two per task, parameters and Adam moments LDS-resident: the work split, the tile layout and every phase are the
// shared tower functions of pgm_ppo_tower.hpp (as ppo_update_cat_kernel / ppo_update_ln_kernel); loss terms,
// clip_grad_norm_ and Adam are pgm_ppo_terms.hpp's.
//
// Padding: the image holds W1t rows o..31, head rows / biases NQ..7 and (Categorical, critic) the logstd slots as
// zeros that map to no flat index (any_img_to_flat returns -1) and are never stored; the gathered row has a fixed
// column map with the columns past the true dims zero.  A zero W1t row meets a zero input column, a zero head row a
// zero dL/d(output): every padding gradient is exactly zero, so Adam keeps the slot at zero and the gradient norm sees
// only true parameters.  The loss loops run over the true a and k.
//
// The Categorical actor loss and entropy are those of pgm_ppo_cat.hip; the Gaussian log-prob, the logstd gradient
// slots and the 1 / std^2 refresh after Adam are those of pgm_ppo_ln.hip's Gaussian loss.
#include <stdio.h>
#include <stdlib.h>

#include "pgm_anydims.hpp"
#include "pgm_ppo_tower.hpp"

PGM_STAMP_UNIT(any)

namespace pgm {

constexpr int QM = AM;  // head outputs of the image (AM >= KM)

struct AnyImg {
    float W1t[OM][H];
    float W2t[H][SCR];
    float Wh[QM][H];
    float b1[H], b2[H], bh[QM], logstd[AM];
};

struct AnyLay {  // plain Layout (a Categorical layout has the same first twelve tensors and no logstd)
    int32_t off[PGM_NUM_PARAM_TENSORS];
    int32_t total;
    int o, a, k, cat;
};

// image slot -> flat parameter index, -1 for padding / unused slots
__device__ __forceinline__ int any_img_to_flat(int i, int m, const AnyLay& L) {
    constexpr int s1 = OM * H, s2 = s1 + H * SCR, s3 = s2 + QM * H, s4 = s3 + H, s5 = s4 + H, s6 = s5 + QM,
                  s7 = s6 + AM;
    const int NQ = m == 0 ? L.k : L.a;
    if (i < s1) return i < L.o * H ? L.off[m ? PGM_P_ACTOR_W1 : PGM_P_CRITIC_W1] + i : -1;
    if (i < s2) {
        const int j = i - s1, in = j / SCR, u = j - in * SCR;
        return u < H ? L.off[m ? PGM_P_ACTOR_W2 : PGM_P_CRITIC_W2] + in * H + u : -1;
    }
    if (i < s3) {  // reference head weight [NQ][H] stored transposed [H][NQ]
        const int j = i - s2, q = j / H, u = j - q * H;
        return q < NQ ? L.off[m ? PGM_P_MEAN_W : PGM_P_VALUE_W] + u * NQ + q : -1;
    }
    if (i < s4) return L.off[m ? PGM_P_ACTOR_B1 : PGM_P_CRITIC_B1] + (i - s3);
    if (i < s5) return L.off[m ? PGM_P_ACTOR_B2 : PGM_P_CRITIC_B2] + (i - s4);
    if (i < s6) return (i - s5) < NQ ? L.off[m ? PGM_P_MEAN_B : PGM_P_VALUE_B] + (i - s5) : -1;
    if (i < s7) return m && !L.cat && (i - s6) < L.a ? L.off[PGM_P_LOGSTD] + (i - s6) : -1;
    return -1;
}

using AnyArgs = TowerArgs<AnyLay>;

// gathered row, fixed columns: obs [0, 32) | action [32, 40) | old logp | adv | old value [42, 45) | return [45, 48)
constexpr int cA = OM, cLp = OM + AM, cAdv = cLp + 1, cV = cAdv + 1, cR = cV + KM, NCA = cR + KM;

struct AnySmem : TowerSmem<AnyImg, NCA, QM> {
    float dls[4][TS][QM];  // per-wave per-sample dL/d(logstd) of the current tile (Gaussian actor)
    float aiv[AM];         // Gaussian actor 1 / std^2 = exp(-2 logstd), refreshed by Adam
};

template <bool CAT>
__global__ __launch_bounds__(MT) void ppo_update_any_kernel(AnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Sm = AnySmem;
    auto& S = *reinterpret_cast<Sm*>(smem_raw);
    constexpr int Q = QM, O = OM;
    constexpr int IMG = Sm::IMG, NC = Sm::NC, RW = Sm::RW;
    constexpr int oB1 = O * H + H * SCR + Q * H, oB2 = oB1 + H, oBh = oB2 + H, oLs = oBh + Q;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int o = a.L.o, A = a.L.a, K = a.L.k, AW = CAT ? 1 : A;
    int p, m;
    if (!tower_block(a.P, p, m)) return;
    const TowerTask<AnyArgs> k(a, p, m, o, AW, K);
    const int NQ = m == 0 ? K : A;
    const float escale = a.hp.entropy_coef / (float)k.mb;

    auto& W = S.Pm;
    float* Pf = &W.W1t[0][0];
    auto to_flat = [&](int i) { return any_img_to_flat(i, m, a.L); };
    if (!CAT && t < AM) S.aiv[t] = t < A ? expf(-2.f * k.P[a.L.off[PGM_P_LOGSTD] + t]) : 0.f;
    tower_img_load<IMG>(Pf, S.MV, k, to_flat);
    const float* lstd = W.logstd;  // critic / Categorical: zeros, unused

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
            float gls = 0.f;               // lanes 32 + q (Gaussian actor): logstd gradient q
            float lsum = 0.f, esum = 0.f;  // loss and entropy sums of this wave's samples

            for (int tile = w; tile * TS < k.mb; tile += 4) {
                const bool ok = tower_gather_tile<NC, RW>(rt, perm, tile * TS, k.mb, h, c, [&](int idx, int col) {
                    if (col < cA) return col < o ? k.obs[(size_t)idx * o + col] : 0.f;
                    if (col < cLp) return col - cA < AW ? k.actions[(size_t)idx * AW + (col - cA)] : 0.f;
                    if (col == cLp) return k.logp[idx];
                    if (col == cAdv) return k.adv[idx];
                    if (col < cR) return col - cV < K ? k.values[(size_t)idx * K + (col - cV)] : 0.f;
                    return col - cR < K ? k.returns[(size_t)idx * K + (col - cR)] : 0.f;
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
                if (m == 0) {  // value loss over the true k
                    float ls = 0.f;
#pragma unroll
                    for (int q = 0; q < KM; ++q)
                        if (q < K) {
                            const LossTerm v = value_loss_term(outv[q], row[cV + q], row[cR + q], k.clip,
                                                               a.hp.use_clipped_value_loss);
                            ls += v.loss;
                            dO[q] = ok ? k.vscale * v.grad : 0.f;
                        }
                    if (ok && h == 0) lsum += ls;
                } else if constexpr (CAT) {  // Categorical log-prob / entropy, clipped surrogate (pgm_ppo_cat.hip)
                    float zm = outv[0];
#pragma unroll
                    for (int q = 1; q < AM; ++q) zm = q < A ? fmaxf(zm, outv[q]) : zm;
                    float ex[AM], se = 0.f;
#pragma unroll
                    for (int q = 0; q < AM; ++q) {
                        ex[q] = 0.f;
                        if (q < A) {
                            ex[q] = expf(outv[q] - zm);
                            se += ex[q];
                        }
                    }
                    const float lse = zm + logf(se), rse = 1.f / se;
                    const int ai = (int)row[cA];  // the taken action (exact integer in fp32)
                    float pj[AM], lpj[AM], lp = outv[0] - lse, ent = 0.f;
#pragma unroll
                    for (int q = 0; q < AM; ++q) {
                        pj[q] = ex[q] * rse;
                        lpj[q] = outv[q] - lse;
                        if (q < A) {
                            ent = fmaf(-pj[q], lpj[q], ent);
                            lp = ai == q ? lpj[q] : lp;
                        }
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
                    for (int q = 0; q < AM; ++q)
                        if (q < A) dO[q] = dlp * ((ai == q ? 1.f : 0.f) - pj[q]) + es * pj[q] * (lpj[q] + ent);
                } else {  // diagonal Gaussian log-prob, clipped surrogate (pgm_ppo_ln.hip)
                    float lp = 0.f;
#pragma unroll
                    for (int q = 0; q < AM; ++q)
                        if (q < A) {
                            const float diff = row[cA + q] - outv[q];
                            lp += -0.5f * diff * diff * S.aiv[q] - lstd[q] - LOG_SQRT_2PI;
                        }
                    const float ratio = expf(lp - row[cLp]);
                    const LossTerm sg = surrogate_term(ratio, row[cAdv], k.clip);
                    const float dlp = ok ? k.ascale * sg.grad * ratio : 0.f;
                    if (ok && h == 0) lsum += sg.loss;
#pragma unroll
                    for (int q = 0; q < AM; ++q) {
                        float dl = 0.f;
                        if (q < A) {
                            const float diff = row[cA + q] - outv[q];
                            const float iv = S.aiv[q];
                            dO[q] = dlp * diff * iv;
                            dl = dlp * (diff * diff * iv - 1.f);
                        }
                        if (h == 0) S.dls[w][c][q] = dl;
                    }
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
                if (!CAT && h == 1 && m == 1 && c < A) tile_col_add<Q>(gls, &S.dls[w][0][0] + c);
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
                [&](auto acc, bool add) {  // -entropy_coef * d(mean entropy)/d logstd enters once (ppo.py:98)
                    if (h == 1 && c < AM)
                        acc(oLs + c, !CAT && m == 1 && c < A ? gls - (add ? 0.f : a.hp.entropy_coef) : 0.f);
                });
            PGM_STAMP(2);
            if (t == 0) {
                const float ls = sum4(S.red + 8);
                if (m == 0) {
                    st_v += ls * k.vstat;
                } else {
                    st_a += ls * k.astat;
                    if constexpr (CAT) {
                        st_e += sum4(S.red + 12) * k.astat;
                    } else {  // entropy with the logstd of this step (before Adam)
                        float ent = 0.f;
                        for (int q = 0; q < A; ++q) ent += 0.5f + LOG_SQRT_2PI + lstd[q];
                        st_e += ent;
                    }
                }
            }
            tower_clip_adam<IMG>(S.big.G, S.MV, Pf, S.red, a, k, nstep, adam, [&](int i, float pp) {
                if (!CAT && m == 1 && i >= oLs && i < oLs + A) S.aiv[i - oLs] = expf(-2.f * pp);
            });
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

size_t pgm_ppo_update_any_workspace_bytes(const pgm_dims* d) { return d && d->P > 0 ? ppo_flag_bytes(d->P) : 0; }

// Validated before any device work: NULL pointers, check_dims, the range of the family, LN, the minibatch shape.
int pgm_ppo_update_any(const pgm_dims* d, int32_t head, const pgm_ppo_hparams* hp, float* params, float* adam_m,
                       float* adam_v, int32_t* adam_step, const float* lr, const int32_t* perms,
                       const pgm_rollout_buf* rb, float* stats, void* workspace, pgm_stream_t stream) {
    const char* what = "pgm_ppo_update_any";
    if (!d || !hp || !params || !adam_m || !adam_v || !adam_step || !lr || !perms || !rb || !rb->obs || !rb->actions ||
        !rb->logp || !rb->values || !rb->returns || !rb->adv || !stats || !workspace) {
        set_error("%s: null pointer (the workspace of pgm_ppo_update_any_workspace_bytes is required)", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, what)) return rc;
    if (int rc = check_any_dims(d, head, what)) return rc;
    if (d->T < 1 || hp->ppo_epoch < 1 || hp->num_mini_batch < 1 || hp->num_mini_batch > d->T * d->N) {
        set_error("%s: bad shape T=%d N=%d ppo_epoch=%d num_mini_batch=%d", what, d->T, d->N, hp->ppo_epoch,
                  hp->num_mini_batch);
        return PGM_E_SHAPE;
    }
    AnyLay L{};
    if (head) {
        const LayoutCat C = make_layout_cat(d->O, d->A, d->K, d->H);
        for (int i = 0; i < PGM_NUM_PARAM_TENSORS_CAT; ++i) L.off[i] = C.off[i];
        L.total = C.total;
    } else {
        const Layout G = make_layout(d->O, d->A, d->K, d->H);
        for (int i = 0; i < PGM_NUM_PARAM_TENSORS; ++i) L.off[i] = G.off[i];
        L.total = G.total;
    }
    L.o = d->O;
    L.a = d->A;
    L.k = d->K;
    L.cat = head;
    AnyArgs a{d->P, d->N, d->T, L, *hp, params, adam_m, adam_v, adam_step, lr, perms, rb->obs, rb->actions, rb->logp,
              rb->values, rb->returns, rb->adv, stats, (unsigned long long*)workspace, dbg_delay_hook()};
    const char* refusal =
        "pgm_ppo_update_any: the update runs one workgroup per tower and needs 2 P = %d <= %d CUs; shard the tasks "
        "over more GPUs";
    if (head)
        return launch_tower_update<sizeof(AnySmem)>(ppo_update_any_kernel<true>, a, (hipStream_t)stream, what, refusal);
    return launch_tower_update<sizeof(AnySmem)>(ppo_update_any_kernel<false>, a, (hipStream_t)stream, what, refusal);
}

}  // extern "C"
