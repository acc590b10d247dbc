// Scalarised clipped-PPO update for discrete-action policies (Categorical head) on the f32 matrix cores
// (v_mfma_f32_32x32x2_f32, exact fp32): ppo_update_cat_kernel.
//
// The towers are the plain ones (Linear -> tanh, twice; a2c_ppo_acktr/model.py:201-256); the head is the reference's
// Categorical (a2c_ppo_acktr/distributions.py:17-27,54-68): logits z = Linear(actor features), one integer action per
// sample.  Work split of the row-split kernel's one-workgroup-per-tower mode (pgm_ppo_mfma.hip MODE 1), structured as
// ppo_update_ln_kernel: two 256-thread workgroups per task, critic and actor, both on one XCD; the tower's parameters
// AND Adam moments stay in LDS for the whole launch (one HBM read at the start, one write at the end); the only
// coupling inside a minibatch step is the squared gradient norm, exchanged as the tagged 8-byte norm granule of
// pgm_common.hpp (ppo_norm_granule, double-buffered by step parity, the same spin limit and timeout word 2P).
//
// Tiles of 32 samples per wave; samples are the accumulator ROWS (registers), features the COLUMNS (lanes):
//     lane l, register r  <->  (sample rowof(r, l>>5), feature l & 31 of column tile 0 / 1).
// Layer 2 and its backward are the MFMA bulk; with A = 4 actions the head is VALU work on four columns.
//
// Actor head, per sample i with taken action a (the index stored as fp32 in the width-1 action column):
//     p = softmax(z) (max-subtracted), logp = log p_a, H_i = -sum_j p_j log p_j,
//     ratio = exp(logp - old logp), clipped surrogate and tie semantics of the plain kernels (wmin2),
//     dL/dz_j = g_i (1[j = a] - p_j) + (entropy_coef / mb) p_j (log p_j + H_i),
// g_i = dL/dlogp of the surrogate (0 on the clipped branch); the second term is -entropy_coef d(mean H)/dz_j.
// Rows past the end of a ragged minibatch are zero inputs with zero loss gradient and zero entropy.
//
// The minibatch rows are gathered straight from the rollout storage through the permutation (no packed table).
// Value loss, clip_grad_norm_ and Adam are those of the plain kernels (a2c_ppo_acktr/algo/ppo.py:58-115).
#include <stdio.h>
#include <stdlib.h>

#include "pgm_dispatch.hpp"
#include "pgm_ppo_shared.hpp"

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
template <int O, int A, int K>
constexpr int cat_img_floats() { return (int)(sizeof(CatImg<O, A, K>) / sizeof(float)); }

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

struct CatArgs {
    int P, N, T;
    LayoutCat L;
    pgm_ppo_hparams hp;
    float *params, *m, *v;
    int32_t* step;
    const float* lr;
    const int32_t* perms;
    const float *obs, *actions, *logp, *values, *returns, *adv;
    float* stats;
    unsigned long long* ws;  // tagged norm granules + timeout word (2P), zeroed before the launch
    DbgDelay dbg;            // test-only exchange delay (PGM_TEST_DELAY; cycles 0 = off)
};

template <int O, int A, int K>
struct CatSmem {
    static constexpr int Q = qmax<A, K>();
    static constexpr int IMG = cat_img_floats<O, A, K>();
    static constexpr int NC = O + 1 + 2 + 2 * K;  // obs | action index | old logp | adv | old value | return
    static constexpr int RW = NC | 1;             // odd row stride: conflict-free per-sample column reads
    CatImg<O, A, K> Pm;                           // parameters
    float MV[2 * IMG];                            // Adam exp_avg | exp_avg_sq images
    float rows[4][TS][RW];                        // per-wave gathered samples of the current tile
    float dout[4][TS][Q];                         // per-wave dL/d(head output) of the current tile
    float red[16];
    union Big {                                   // transpose tiles during the tiles, the gradient image after
        float scr[4][TS][SCR];
        float G[IMG];
    } big;
};

// blocks of the launch: groups of 16 for 8 tasks, block r of a group = tower (r >> 3) & 1 of task 8 g + (r & 7), so
// a task's two workgroups share an XCD under round-robin dispatch (padding blocks of a partial group exit at once)
inline int cat_grid(int P) { return 16 * ((P + 7) / 8); }

template <int O, int A, int K>
__global__ __launch_bounds__(MT) void ppo_update_cat_kernel(CatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Sm = CatSmem<O, A, K>;
    auto& S = *reinterpret_cast<Sm*>(smem_raw);
    constexpr int Q = qmax<A, K>();
    constexpr int KS1 = (O + 1) / 2;  // k-steps of layer 1
    constexpr int IMG = Sm::IMG, NC = Sm::NC, RW = Sm::RW;
    constexpr int oW2 = O * H, oWh = oW2 + H * SCR, oB1 = oWh + Q * H, oB2 = oB1 + H, oBh = oB2 + H;
    constexpr int cA = O, cLp = O + 1, cAdv = O + 2, cV = O + 3, cR = O + 3 + K;  // columns of a gathered row
    const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int bx = (int)blockIdx.x;
    const int p = 8 * (bx >> 4) + (bx & 7);
    if (p >= a.P) return;
    const int m = (bx >> 3) & 1;  // tower: 0 critic, 1 actor
    const int NQ = m == 0 ? K : A;
    const int N = a.N, T = a.T, B = T * N, BV = (T + 1) * N;
    const int E = a.hp.ppo_epoch, M = a.hp.num_mini_batch;
    const int mb = B / M, nb = B / mb;
    const float clip = a.hp.clip_param;
    const LayoutCat& L = a.L;
    float* __restrict__ P = a.params + (size_t)p * L.total;
    float* __restrict__ Mo = a.m + (size_t)p * L.total;
    float* __restrict__ Vo = a.v + (size_t)p * L.total;
    const float* obs = a.obs + (size_t)p * BV * O;
    const float* actions = a.actions + (size_t)p * B;  // width 1
    const float* logp = a.logp + (size_t)p * B;
    const float* advs = a.adv + (size_t)p * B;
    const float* values = a.values + (size_t)p * BV * K;
    const float* returns = a.returns + (size_t)p * BV * K;

    // ---- parameter and Adam moment images from the flat HBM vectors
    float* Pf = &S.Pm.W1t[0][0];
    for (int i = t; i < IMG; i += MT) {
        const int f = cat_img_to_flat<O, A, K>(i, m, L);
        Pf[i] = f >= 0 ? P[f] : 0.f;
        S.MV[i] = f >= 0 ? Mo[f] : 0.f;
        S.MV[IMG + i] = f >= 0 ? Vo[f] : 0.f;
    }
    __syncthreads();
    auto& W = S.Pm;

    const int step0 = a.step[p];
    const double lr = a.lr[p];
    const float b1c = a.hp.beta1, b2c = a.hp.beta2, eps = a.hp.adam_eps;
    const float vscale = a.hp.value_loss_coef * 0.5f / (float)(mb * K);
    const float ascale = -1.f / (float)mb;
    const float escale = a.hp.entropy_coef / (float)mb;
    const float vstat = 0.5f / (float)(mb * K), astat = 1.f / (float)mb;  // loss statistics scales
    float st_v = 0.f, st_a = 0.f, st_e = 0.f;
    int nstep = 0;
    double b1p = pow((double)b1c, (double)step0), b2p = pow((double)b2c, (double)step0);
    float* scr = &S.big.scr[w][0][0];
    float* rt = &S.rows[w][0][0];
    auto rowf = [&](int cs, int k) { return rt[cs * RW + k]; };
    float* G = S.big.G;
    PGM_STAMP_DECL

    for (int e = 0; e < E; ++e) {
        const int32_t* perm = a.perms + (size_t)e * B;
        for (int bb = 0; bb < nb; ++bb) {
            f32x16 gW2[2][2], gW1[2];  // [in tile][out tile], [out tile] (O <= 32: one in tile)
            float gWh[2][Q], gB1[2], gB2[2];
            float gsm = 0.f;  // lanes q < Q of half 0: head-bias gradient q
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) gW2[i][j] = f32x16{0};
                gW1[i] = f32x16{0};
                gB1[i] = gB2[i] = 0.f;
#pragma unroll
                for (int q = 0; q < Q; ++q) gWh[i][q] = 0.f;
            }
            float lsum = 0.f, esum = 0.f;  // loss and entropy sums of this wave's samples

            for (int tile = w; tile * TS < mb; tile += 4) {
                const int ts0 = tile * TS;
                // ---- gather the tile's samples: lane (h, c) fills half h of sample c's columns; rows past the
                // minibatch are zero inputs
                {
                    const bool okr = ts0 + c < mb;
                    const int idx = okr ? perm[bb * mb + ts0 + c] : 0;
                    for (int k = h; k < NC; k += 2) {
                        float x = 0.f;
                        if (okr) {
                            if (k < O) x = obs[(size_t)idx * O + k];
                            else if (k == cA) x = actions[idx];
                            else if (k == cLp) x = logp[idx];
                            else if (k == cAdv) x = advs[idx];
                            else if (k < cR) x = values[(size_t)idx * K + (k - cV)];
                            else x = returns[(size_t)idx * K + (k - cR)];
                        }
                        rt[c * RW + k] = x;
                    }
                }
                wave_lds_fence();
                PGM_STAMP(0);
                // ---- layer 1: H1[s][u] = tanh(X[s][:] . W1t[:][u] + b1[u])
                f32x16 z[2] = {f32x16{0}, f32x16{0}};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    const int k = 2 * ks + h;
                    const float av = k < O ? rowf(c, k) : 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb) z[hb] = mfma(av, k < O ? W.W1t[k][hb * TS + c] : 0.f, z[hb]);
                }
                f32x16 H1[2];
#pragma unroll
                for (int hb = 0; hb < 2; ++hb) tanh_bias_pk<16>(z[hb], W.b1[hb * TS + c], H1[hb]);
#pragma unroll
                for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) scr[rowof(r, h) * SCR + hb * TS + c] = H1[hb][r];
                wave_lds_fence();
                // ---- layer 2: H2[s][o] = tanh(H1[s][:] . W2t[:][o] + b2[o])   (A from the transpose tile)
                z[0] = z[1] = f32x16{0};
#pragma unroll 8
                for (int ks = 0; ks < H / 2; ++ks) {
                    const int k = 2 * ks + h;
                    const float av = scr[c * SCR + k];
#pragma unroll
                    for (int ob = 0; ob < 2; ++ob) z[ob] = mfma(av, W.W2t[k][ob * TS + c], z[ob]);
                }
                f32x16 H2[2];
#pragma unroll
                for (int ob = 0; ob < 2; ++ob) tanh_bias_pk<16>(z[ob], W.b2[ob * TS + c], H2[ob]);
                PGM_STAMP(4);
                wave_lds_fence();  // every lane finished reading the H1 tile
#pragma unroll
                for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) scr[rowof(r, h) * SCR + ob * TS + c] = H2[ob][r];
                wave_lds_fence();
                // ---- heads on the VALU: lane = sample c, half h sums units [32h, 32h+32)
                float outv[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) outv[q] = 0.f;
#pragma unroll 8
                for (int u = 0; u < TS; ++u) {
                    const float hv = scr[c * SCR + h * TS + u];
#pragma unroll
                    for (int q = 0; q < Q; ++q) outv[q] = fmaf(hv, W.Wh[q][h * TS + u], outv[q]);
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) outv[q] = half_sum(outv[q]) + W.bh[q];
                PGM_STAMP(16);
                // ---- per-sample loss gradients (ppo.py:80-96); both halves compute the same sample
                const bool ok = ts0 + c < mb;
                float dO[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) dO[q] = 0.f;
                if (m == 0) {  // value loss
                    float ls = 0.f;
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        const float V = outv[q], Vold = rowf(c, cV + q);
                        const float R = rowf(c, cR + q);
                        float gv;
                        if (a.hp.use_clipped_value_loss) {
                            const float dv = V - Vold;
                            const float vc = Vold + fminf(fmaxf(dv, -clip), clip);
                            const float l1 = (V - R) * (V - R), l2 = (vc - R) * (vc - R);
                            const float inr = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
                            gv = wmax2(l1, l2) * 2.f * (V - R) + wmax2(l2, l1) * 2.f * (vc - R) * inr;
                            ls += fmaxf(l1, l2);
                        } else {
                            gv = 2.f * (V - R);
                            ls += (R - V) * (R - V);
                        }
                        dO[q] = ok ? vscale * gv : 0.f;
                    }
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
                    const int ai = (int)rowf(c, cA);  // the taken action (exact integer in fp32)
                    float pj[A], lpj[A], lp = outv[0] - lse, ent = 0.f;
#pragma unroll
                    for (int q = 0; q < A; ++q) {
                        pj[q] = ex[q] * rse;
                        lpj[q] = outv[q] - lse;
                        ent = fmaf(-pj[q], lpj[q], ent);
                        lp = ai == q ? lpj[q] : lp;
                    }
                    const float ratio = expf(lp - rowf(c, cLp));
                    const float ad = rowf(c, cAdv);
                    const float s1 = ratio * ad;
                    const float s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * ad;
                    const float inr = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? 1.f : 0.f;
                    const float gr = ad * (wmin2(s1, s2) + wmin2(s2, s1) * inr);
                    const float dlp = ok ? ascale * gr * ratio : 0.f;
                    const float es = ok ? escale : 0.f;
                    if (ok && h == 0) {
                        lsum += -fminf(s1, s2);
                        esum += ent;
                    }
#pragma unroll
                    for (int q = 0; q < A; ++q)
                        dO[q] = dlp * ((ai == q ? 1.f : 0.f) - pj[q]) + es * pj[q] * (lpj[q] + ent);
                }
                if (h == 0) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) S.dout[w][c][q] = dO[q];
                }
                PGM_STAMP(17);
                wave_lds_fence();
                // per-column sums of the tile: lane q of half 0 sums dO[.][q]
                if (h == 0 && c < Q) {
                    const float* src = &S.dout[w][0][0] + c;
#pragma unroll 8
                    for (int cc = 0; cc < TS; ++cc) gsm += src[cc * Q];
                }
                PGM_STAMP(5);
                // ---- head-weight grads (VALU, C layout): gWh[ob][q] += sum_r H2[s][u] dO[s][q]
#pragma unroll
                for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int s = rowof(r, h);
#pragma unroll
                        for (int q = 0; q < Q; ++q) gWh[ob][q] = fmaf(H2[ob][r], S.dout[w][s][q], gWh[ob][q]);
                    }
                // ---- dH2 = dO . Wh  (MFMA; A = this lane's sample, k = head output)
                z[0] = z[1] = f32x16{0};
#pragma unroll
                for (int ks = 0; ks < (Q + 1) / 2; ++ks) {
                    const int q = 2 * ks + h;
                    const float av = h ? (2 * ks + 1 < Q ? dO[2 * ks + 1] : 0.f) : dO[2 * ks];
#pragma unroll
                    for (int ob = 0; ob < 2; ++ob) z[ob] = mfma(av, q < Q ? W.Wh[q][ob * TS + c] : 0.f, z[ob]);
                }
                // ---- dZ2 = dH2 (1 - H2^2); the bias gradient sums it over the samples (registers), per lane
                f32x16 dZ2[2];
#pragma unroll
                for (int ob = 0; ob < 2; ++ob) {
                    dtanh_pk<16>(z[ob], H2[ob], dZ2[ob]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) gB2[ob] += dZ2[ob][r];
                }
                PGM_STAMP(6);
                // ---- dH1 = dZ2 W2  (A = dZ2 through the transpose tile, B = W2t[in][o] column)
                wave_lds_fence();  // heads finished reading the H2 tile
#pragma unroll
                for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) scr[rowof(r, h) * SCR + ob * TS + c] = dZ2[ob][r];
                wave_lds_fence();
                z[0] = z[1] = f32x16{0};
#pragma unroll 8
                for (int ks = 0; ks < H / 2; ++ks) {
                    const int k = 2 * ks + h;  // output unit o
                    const float av = scr[c * SCR + k];
#pragma unroll
                    for (int ib = 0; ib < 2; ++ib) z[ib] = mfma(av, W.W2t[ib * TS + c][k], z[ib]);
                }
                // ---- dW2^T[in][o] += H1^T dZ2: straight from the C-layout registers
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                        for (int ob = 0; ob < 2; ++ob) gW2[ib][ob] = mfma(H1[ib][r], dZ2[ob][r], gW2[ib][ob]);
                // ---- dZ1 = dH1 (1 - H1^2) (in z), bias gradient
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) {
                    dtanh_pk<16>(z[ib], H1[ib], z[ib]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) gB1[ib] += z[ib][r];
                }
                // ---- dW1^T[k][u] += X^T dZ1  (A = X[s(r)][k = lane], B = dZ1 reg r)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float av = c < O ? rowf(rowof(r, h), c) : 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb) gW1[hb] = mfma(av, z[hb][r], gW1[hb]);
                }
                wave_lds_fence();  // dH1 finished reading the dZ2 tile, dW1 the rows, before the next tile's writes
                PGM_STAMP(7);
            }  // tiles

            // ---- combine the lane halves of the per-column partial sums
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                gB1[i] = half_sum(gB1[i]);
                gB2[i] = half_sum(gB2[i]);
#pragma unroll
                for (int q = 0; q < Q; ++q) gWh[i][q] = half_sum(gWh[i][q]);
            }
            lsum = wave_sum64(lsum);
            esum = wave_sum64(esum);
            if (l == 0) {
                S.red[8 + w] = lsum;
                S.red[12 + w] = esum;
            }
            lds_sync_m();  // every wave's tiles done: the gradient image overwrites the transpose tiles
            PGM_STAMP(12);

            // ---- gradient image: wave 0 stores its partials (and the zeros of the padding slots), waves 1..3 add
            // theirs in order, one barrier per round: every element is ((w0 + w1) + w2) + w3, deterministic
            for (int round = 0; round < 4; ++round) {
                if (w == round) {
                    const bool add = round != 0;
                    auto acc = [&](int idx, float val) { G[idx] = add ? G[idx] + val : val; };
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                acc(oW2 + (i * TS + rowof(r, h)) * SCR + ob * TS + c, gW2[i][ob][r]);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {  // rows k >= O of dW1 are exactly zero (A operand 0)
                            const int k = rowof(r, h);
                            if (k < O) acc(k * H + i * TS + c, gW1[i][r]);
                        }
                        if (h == 0) {  // per-unit sums of unit block i
                            acc(oB1 + i * TS + c, gB1[i]);
                            acc(oB2 + i * TS + c, gB2[i]);
#pragma unroll
                            for (int q = 0; q < Q; ++q) acc(oWh + q * H + i * TS + c, q < NQ ? gWh[i][q] : 0.f);
                        }
                    }
                    if (h == 0 && c < Q) acc(oBh + c, c < NQ ? gsm : 0.f);
                    if (!add) G[oW2 + l * SCR + H] = 0.f;  // W2 padding column
                }
                lds_sync_m();
            }
            PGM_STAMP(2);
            // ---- clip_grad_norm_ over every parameter (padding slots hold zeros)
            float sq = 0.f;
            for (int i = t; i < IMG; i += MT) sq = fmaf(G[i], G[i], sq);
            sq = wave_sum64(sq);
            if (l == 0) S.red[w] = sq;
            lds_sync_m();
            PGM_STAMP(8);
            float total = (S.red[0] + S.red[1]) + (S.red[2] + S.red[3]);
            if (t == 0) {  // tagged 8-byte granule hand-off with the other tower's workgroup
                const unsigned tag = (unsigned)(nstep + 1);
                unsigned long long* ws = a.ws + ppo_norm_granule(a.P, p, 0, 0, nstep & 1);
                __hip_atomic_store(ws + m, ((unsigned long long)tag << 32) | __float_as_uint(total), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                dbg_delay(a.dbg, nstep, 2);
                unsigned long long x = 0;
                const bool failed = __hip_atomic_load(a.ws + 2 * a.P, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (unsigned spins = 0; !failed; ++spins) {
                    x = __hip_atomic_load(ws + (1 - m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(x >> 32) == tag) break;
                    if (spins > (1u << 26)) {  // partner never arrived: flag the launch as failed
                        __hip_atomic_store(a.ws + 2 * a.P, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        x = 0;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                const float other = __uint_as_float((unsigned)x);
                S.red[4] = m == 0 ? total + other : other + total;  // critic + actor in both workgroups
            }
            lds_sync_m();
            total = S.red[4];
            PGM_STAMP(9);
            const float coef = clip_coef(a.hp.max_grad_norm, total);
            if (t == 0) {
                const float ls = (S.red[8] + S.red[9]) + (S.red[10] + S.red[11]);
                if (m == 0) {
                    st_v += ls * vstat;
                } else {
                    st_a += ls * astat;
                    st_e += ((S.red[12] + S.red[13]) + (S.red[14] + S.red[15])) * astat;
                }
            }
            // ---- Adam, one flat pass over the images (padding: g = m = v = 0 keeps p = 0)
            ++nstep;
            const double b1n = b1p * (double)b1c, b2n = b2p * (double)b2c;
            const float step_size = (float)(lr / (1.0 - b1n));
            const float inv_bc2s = 1.f / (float)sqrt(1.0 - b2n);
            b1p = b1n;
            b2p = b2n;
            for (int i = t; i < IMG; i += MT) {
                const float gc = G[i] * coef;
                float mm = S.MV[i], vv = S.MV[IMG + i], pp = Pf[i];
                mm = mm + (1.f - b1c) * (gc - mm);
                vv = vv * b2c + (1.f - b2c) * (gc * gc);
                // torch: p -= step_size * m / (sqrt(v) / sqrt(bc2) + eps); hardware sqrt / rcp
                const float den = __builtin_amdgcn_sqrtf(vv) * inv_bc2s + eps;
                pp -= step_size * mm * __builtin_amdgcn_rcpf(den);
                S.MV[i] = mm;
                S.MV[IMG + i] = vv;
                Pf[i] = pp;
            }
            lds_sync_m();  // parameters updated before the next minibatch; G region reused as transpose tiles
            PGM_STAMP(3);
        }  // minibatches
    }      // epochs
    // ---- write back the parameters and the moments
    for (int i = t; i < IMG; i += MT) {
        const int f = cat_img_to_flat<O, A, K>(i, m, L);
        if (f < 0) continue;
        P[f] = Pf[i];
        Mo[f] = S.MV[i];
        Vo[f] = S.MV[IMG + i];
    }
    if (t == 0) {
        const float n = (float)(E * M);
        if (m == 0) {
            a.stats[p * 3 + 0] = st_v / n;
        } else {
            a.step[p] = step0 + nstep;
            a.stats[p * 3 + 1] = st_a / n;
            a.stats[p * 3 + 2] = st_e / n;
        }
    }
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
        constexpr size_t smem = sizeof(CatSmem<O, A, K>);
        static_assert(smem <= 160 * 1024, "categorical update LDS image exceeds 160 KiB");
        static_assert(smem > 80 * 1024, "one workgroup per CU: the residency argument needs > 80 KiB LDS");
        const int cus = device_cu_count();
        if (2 * d->P > cus) {
            set_error("pgm_ppo_update_cat: the update runs one workgroup per tower and needs 2 P = %d <= %d CUs; "
                      "shard the tasks over more GPUs", 2 * d->P, cus);
            return PGM_E_UNSUPPORTED;
        }
        auto kern = ppo_update_cat_kernel<O, A, K>;
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return hip_fail(e, "pgm_ppo_update_cat");
        // the workgroups exchange through spin-waits: the 2 P working ones must be resident together (the
        // padding blocks of the last group exit at once)
        if (int rc = check_coresident((const void*)kern, MT, smem, 2 * d->P, "pgm_ppo_update_cat")) return rc;
        const size_t zb = ppo_flag_bytes(d->P);  // norm granules + timeout word start at tag 0
        if (!ws_take_zeroed(a.ws, zb)) {
            e = hipMemsetAsync(a.ws, 0, zb, (hipStream_t)stream);
            if (e != hipSuccess) return hip_fail(e, "pgm_ppo_update_cat (workspace reset)");
        }
        hipLaunchKernelGGL(kern, dim3(cat_grid(d->P)), dim3(MT), smem, (hipStream_t)stream, a);
        return launch_status("pgm_ppo_update_cat");
    });
}

}  // extern "C"
