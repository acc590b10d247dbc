// The one-workgroup-per-tower PPO update (ppo_update_ln_kernel, ppo_update_cat_kernel) as shared device functions.
//
// Two 256-thread workgroups per task, critic and actor; a tower's parameters and Adam moments live in LDS as one flat
// image for the whole launch; tiles of 32 samples per wave on the f32 MFMA, samples on accumulator rows, features on
// lanes (pgm_mfma.hpp).  A kernel supplies what is its own -- the image struct and its slot map, the row columns, the
// activation and its backward, the actor loss, the extra image slots -- as arguments; nothing here knows which
// kernel calls it.  Summation orders are fixed: waves ((w0 + w1) + w2) + w3, (red0 + red1) + (red2 + red3), critic +
// actor.
#pragma once
#include "pgm_mfma.hpp"

namespace pgm {

template <class LayoutT>
struct TowerArgs {
    int P, N, T;
    LayoutT L;
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

// LDS of one workgroup around the kernel's image Img (W1t | W2t | Wh first, then its own slots): the image, both Adam
// moment images, the per-wave row and dL/d(head output) tables (NC gathered columns per sample, Q head outputs)
template <class Img, int NC_, int Q>
struct TowerSmem {
    static constexpr int IMG = (int)(sizeof(Img) / sizeof(float));
    static constexpr int NC = NC_;
    static constexpr int RW = NC | 1;  // odd row stride: conflict-free per-sample column reads
    Img Pm;                            // parameters
    float MV[2 * IMG];                 // Adam exp_avg | exp_avg_sq images
    float rows[4][TS][RW];             // per-wave gathered samples of the current tile
    float dout[4][TS][Q];              // per-wave dL/d(head output) of the current tile
    float red[16];
    union Big {                        // transpose tiles during the tiles, the gradient image after
        float scr[4][TS][SCR];
        float G[IMG];
    } big;
};

// blocks of the launch: groups of 16 for 8 tasks, block r of a group = tower (r >> 3) & 1 of task 8 g + (r & 7), so
// a task's two workgroups share an XCD under round-robin dispatch (padding blocks of a partial group exit at once)
inline int tower_grid(int P) { return 16 * ((P + 7) / 8); }
__device__ __forceinline__ bool tower_block(int P, int& p, int& m) {
    const int bx = (int)blockIdx.x;
    p = 8 * (bx >> 4) + (bx & 7);
    m = (bx >> 3) & 1;  // tower: 0 critic, 1 actor
    return p < P;
}

// One workgroup's view of the launch: its task and tower, the minibatch shape, the loss and statistics scales, Adam's
// constants, its slices of the parameter vectors and of the rollout storage (AW: floats per stored action)
template <class Args>
struct TowerTask {
    int p, m, B, E, M, mb, nb, step0;
    float clip, vscale, ascale, vstat, astat, b1, b2, eps;
    double lr;
    float *__restrict__ P, *__restrict__ Mo, *__restrict__ Vo;
    const float *obs, *actions, *logp, *adv, *values, *returns;
    __device__ __forceinline__ TowerTask(const Args& a, int p_, int m_, int O, int AW, int K)
        : p(p_), m(m_), B(a.T * a.N), E(a.hp.ppo_epoch), M(a.hp.num_mini_batch), mb(B / M), nb(B / mb),
          step0(a.step[p_]), clip(a.hp.clip_param), vscale(a.hp.value_loss_coef * 0.5f / (float)(mb * K)),
          ascale(-1.f / (float)mb), vstat(0.5f / (float)(mb * K)), astat(1.f / (float)mb), b1(a.hp.beta1),
          b2(a.hp.beta2), eps(a.hp.adam_eps), lr(a.lr[p_]) {
        const size_t BV = (size_t)(a.T + 1) * a.N;
        P = a.params + (size_t)p * a.L.total;
        Mo = a.m + (size_t)p * a.L.total;
        Vo = a.v + (size_t)p * a.L.total;
        obs = a.obs + p * BV * O;
        actions = a.actions + (size_t)p * B * AW;
        logp = a.logp + (size_t)p * B;
        adv = a.adv + (size_t)p * B;
        values = a.values + p * BV * K;
        returns = a.returns + p * BV * K;
    }
};

__device__ __forceinline__ float sum4(const float* r) { return (r[0] + r[1]) + (r[2] + r[3]); }

// ---- parameter and Adam moment images <-> the flat HBM vectors (to_flat: image slot -> flat index, -1 = padding)
template <int IMG, class Args, class ToFlat>
__device__ __forceinline__ void tower_img_load(float* Pf, float* MV, const TowerTask<Args>& k, ToFlat to_flat) {
    for (int i = threadIdx.x; i < IMG; i += MT) {
        const int f = to_flat(i);
        Pf[i] = f >= 0 ? k.P[f] : 0.f;
        MV[i] = f >= 0 ? k.Mo[f] : 0.f;
        MV[IMG + i] = f >= 0 ? k.Vo[f] : 0.f;
    }
    __syncthreads();
}
template <int IMG, class Args, class ToFlat>
__device__ __forceinline__ void tower_img_store(const float* Pf, const float* MV, const TowerTask<Args>& k,
                                                ToFlat to_flat) {
    for (int i = threadIdx.x; i < IMG; i += MT) {
        const int f = to_flat(i);
        if (f < 0) continue;
        k.P[f] = Pf[i];
        k.Mo[f] = MV[i];
        k.Vo[f] = MV[IMG + i];
    }
}

// per-wave gradient partials of one minibatch (value-initialise: zeros)
template <int Q>
struct TowerGrads {
    f32x16 gW2[2][2], gW1[2];  // [in tile][out tile], [out tile] (O <= 32: one in tile)
    float gWh[2][Q];
    float gsm;  // lanes q < Q of half 0: head-bias gradient q (half 1 is the kernel's own)
};

// ---- gather the samples of the tile at ts0 of a minibatch (perm: its mb rollout indices): lane (h, c) fills half h
// of sample c's columns (col(idx, k): column k of rollout sample idx); rows past the minibatch are zero inputs.
// Returns whether lane c's sample is inside the minibatch.
template <int NC, int RW, class Col>
__device__ __forceinline__ bool tower_gather_tile(float* rt, const int32_t* perm, int ts0, int mb, int h, int c,
                                                  Col col) {
    const bool ok = ts0 + c < mb;
    const int idx = ok ? perm[ts0 + c] : 0;
    for (int k = h; k < NC; k += 2) rt[c * RW + k] = ok ? col(idx, k) : 0.f;
    wave_lds_fence();
    return ok;
}

// C-layout registers -> this wave's transpose tile
__device__ __forceinline__ void tile_to_scr(float* scr, const f32x16 (&v)[2], int h, int c) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) scr[rowof(r, h) * SCR + b * TS + c] = v[b][r];
}
// acc += a column of a [TS][Q] per-wave table, sample after sample (one running sum over all of a wave's tiles)
template <int Q>
__device__ __forceinline__ void tile_col_add(float& acc, const float* src) {
#pragma unroll 8
    for (int cc = 0; cc < TS; ++cc) acc += src[cc * Q];
}

// ---- forward of one tile: layer 1 and 2 on the MFMA with the kernel's activation (act(z, Hout): pre-activations in
// two column tiles -> layer output; it may keep what its backward needs), heads on the VALU
template <int O, int Q, int RW, class Img, class Act1, class Act2>
__device__ __forceinline__ void tower_forward_tile(const float* rt, float* scr, const Img& W, int h, int c,
                                                   f32x16 (&H1)[2], f32x16 (&H2)[2], float (&outv)[Q], Act1 act1,
                                                   Act2 act2) {
    // layer 1: Z1[s][u] = X[s][:] . W1t[:][u]
    f32x16 z[2] = {f32x16{0}, f32x16{0}};
#pragma unroll
    for (int ks = 0; ks < (O + 1) / 2; ++ks) {
        const int k = 2 * ks + h;
        const float av = k < O ? rt[c * RW + k] : 0.f;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) z[hb] = mfma(av, k < O ? W.W1t[k][hb * TS + c] : 0.f, z[hb]);
    }
    act1(z, H1);
    tile_to_scr(scr, H1, h, c);
    wave_lds_fence();
    // layer 2: Z2[s][o] = H1[s][:] . W2t[:][o]   (A from the transpose tile)
    z[0] = z[1] = f32x16{0};
#pragma unroll 8
    for (int ks = 0; ks < H / 2; ++ks) {
        const int k = 2 * ks + h;
        const float av = scr[c * SCR + k];
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) z[ob] = mfma(av, W.W2t[k][ob * TS + c], z[ob]);
    }
    act2(z, H2);
    wave_lds_fence();  // every lane finished reading the H1 tile
    tile_to_scr(scr, H2, h, c);
    wave_lds_fence();
    // heads on the VALU: lane = sample c, half h sums units [32h, 32h+32)
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
}

// ---- critic: dL/dV of the K value outputs (old values at vold[q], returns at ret[q]) into dO; the sample's loss sum
template <int K, int Q>
__device__ __forceinline__ float tower_value_loss(float (&dO)[Q], const float (&outv)[Q], const float* vold,
                                                  const float* ret, float clip, bool clipped, bool ok, float vscale) {
    float ls = 0.f;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const LossTerm v = value_loss_term(outv[q], vold[q], ret[q], clip, clipped);
        ls += v.loss;
        dO[q] = ok ? vscale * v.grad : 0.f;
    }
    return ls;
}

// ---- backward of one tile from dO (this lane's sample; zero past the minibatch): head-weight and head-bias
// gradients, dH2, the kernel's activation backward (dact(z, Hout): dL/d(layer output) -> dL/d(pre-activation) in
// place, accumulating its own parameter gradients), dH1, dW2, dW1
template <int O, int Q, int RW, class Img, class DAct2, class DAct1>
__device__ __forceinline__ void tower_backward_tile(TowerGrads<Q>& g, const float (&dO)[Q], float* dout,
                                                    const float* rt, float* scr, const Img& W, const f32x16 (&H1)[2],
                                                    const f32x16 (&H2)[2], int h, int c, DAct2 dact2, DAct1 dact1) {
    if (h == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) dout[c * Q + q] = dO[q];
    }
    wave_lds_fence();
    if (h == 0 && c < Q) tile_col_add<Q>(g.gsm, dout + c);  // lane q of half 0 sums dO[.][q]
    // head-weight grads (VALU, C layout): gWh[ob][q] += sum_r H2[s][u] dO[s][q]
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int s = rowof(r, h);
#pragma unroll
            for (int q = 0; q < Q; ++q) g.gWh[ob][q] = fmaf(H2[ob][r], dout[s * Q + q], g.gWh[ob][q]);
        }
    // dH2 = dO . Wh  (MFMA; A = this lane's sample, k = head output)
    f32x16 z[2] = {f32x16{0}, f32x16{0}};
#pragma unroll
    for (int ks = 0; ks < (Q + 1) / 2; ++ks) {
        const int q = 2 * ks + h;
        const float av = h ? (2 * ks + 1 < Q ? dO[2 * ks + 1] : 0.f) : dO[2 * ks];
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) z[ob] = mfma(av, q < Q ? W.Wh[q][ob * TS + c] : 0.f, z[ob]);
    }
    dact2(z, H2);
    const f32x16 dZ2[2] = {z[0], z[1]};
    // dH1 = dZ2 W2  (A = dZ2 through the transpose tile, B = W2t[in][o] column)
    wave_lds_fence();  // heads finished reading the H2 tile
    tile_to_scr(scr, dZ2, h, c);
    wave_lds_fence();
    z[0] = z[1] = f32x16{0};
#pragma unroll 8
    for (int ks = 0; ks < H / 2; ++ks) {
        const int k = 2 * ks + h;  // output unit o
        const float av = scr[c * SCR + k];
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) z[ib] = mfma(av, W.W2t[ib * TS + c][k], z[ib]);
    }
    // dW2^T[in][o] += H1^T dZ2: straight from the C-layout registers
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) g.gW2[ib][ob] = mfma(H1[ib][r], dZ2[ob][r], g.gW2[ib][ob]);
    dact1(z, H1);
    // dW1^T[k][u] += X^T dZ1  (A = X[s(r)][k = lane], B = dZ1 reg r)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float av = c < O ? rt[rowof(r, h) * RW + c] : 0.f;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) g.gW1[hb] = mfma(av, z[hb][r], g.gW1[hb]);
    }
    wave_lds_fence();  // dH1 finished reading the dZ2 tile, dW1 the rows, before the next tile's writes
}

// ---- gradient image G (W1t | W2t | Wh | the kernel's slots from oWh + Q H on, head bias at oBh): wave 0 stores its
// partials (and the zeros of the padding slots), waves 1..3 add theirs in order, one barrier per round, so every
// element is ((w0 + w1) + w2) + w3.  units(acc, i) places the kernel's per-unit sums of unit block i (lanes of half
// 0), rest(acc, add) whatever else it owns.  Call after a workgroup barrier (G overlays the transpose tiles).
template <int O, int Q, class Units, class Rest>
__device__ __forceinline__ void tower_reduce_image(float* G, TowerGrads<Q>& g, int NQ, int oBh, Units units,
                                                   Rest rest) {
    constexpr int oW2 = O * H, oWh = oW2 + H * SCR;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < Q; ++q) g.gWh[i][q] = half_sum(g.gWh[i][q]);
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
                        acc(oW2 + (i * TS + rowof(r, h)) * SCR + ob * TS + c, g.gW2[i][ob][r]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // rows k >= O of dW1 are exactly zero (A operand 0)
                    const int k = rowof(r, h);
                    if (k < O) acc(k * H + i * TS + c, g.gW1[i][r]);
                }
                if (h == 0) {
                    units(acc, i);
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc(oWh + q * H + i * TS + c, q < NQ ? g.gWh[i][q] : 0.f);
                }
            }
            if (h == 0 && c < Q) acc(oBh + c, c < NQ ? g.gsm : 0.f);
            rest(acc, add);
            if (!add) G[oW2 + l * SCR + H] = 0.f;  // W2 padding column
        }
        lds_sync_m();
    }
}

// ---- the optimiser step on a reduced gradient image: clip_grad_norm_ over both towers (this tower's sum of squares,
// padding slots hold zeros; the tagged granule hand-off with the other tower's workgroup), then Adam as one flat pass
// over the images (padding: g = m = v = 0 keeps p = 0); on_elem(i, p) sees every new value.  red: 5 floats of LDS.
template <int IMG, class Args, class OnElem>
__device__ __forceinline__ void tower_clip_adam(const float* G, float* MV, float* Pf, float* red, const Args& a,
                                                const TowerTask<Args>& k, int& nstep, AdamScalars& adam,
                                                OnElem on_elem) {
    const int t = threadIdx.x;
    float sq = 0.f;
    for (int i = t; i < IMG; i += MT) sq = fmaf(G[i], G[i], sq);
    sq = wave_sum64(sq);
    if ((t & 63) == 0) red[t >> 6] = sq;
    lds_sync_m();
    if (t == 0)
        red[4] = tower_norm_exchange(a.ws + ppo_norm_granule(a.P, k.p, 0, 0, nstep & 1), k.m, (unsigned)(nstep + 1),
                                     sum4(red), a.ws + 2 * a.P, a.dbg, nstep);
    lds_sync_m();
    const float coef = clip_coef(a.hp.max_grad_norm, red[4]);
    ++nstep;
    adam.advance(k.lr, k.b1, k.b2);
    for (int i = t; i < IMG; i += MT) {
        float mm = MV[i], vv = MV[IMG + i], pp = Pf[i];
        adam_step(G[i], coef, mm, vv, pp, k.b1, k.b2, adam.step_size, adam.inv_bc2s, k.eps);
        MV[i] = mm;
        MV[IMG + i] = vv;
        Pf[i] = pp;
        on_elem(i, pp);
    }
    lds_sync_m();  // parameters updated before the next minibatch; G region reused as transpose tiles
}

// the launch's statistics (means over the E M steps) and the step counter, by thread 0 of each tower
template <class Args>
__device__ __forceinline__ void tower_write_stats(const Args& a, const TowerTask<Args>& k, int nstep, float st_v,
                                                  float st_a, float st_e) {
    const float n = (float)(k.E * k.M);
    if (k.m == 0) {
        a.stats[k.p * 3 + 0] = st_v / n;
    } else {
        a.step[k.p] = k.step0 + nstep;
        a.stats[k.p * 3 + 1] = st_a / n;
        a.stats[k.p * 3 + 2] = st_e / n;
    }
}

// ---- host: launch a tower-update kernel on tower_grid(P) blocks.  SMEM in (80, 160] KiB: one workgroup per CU, so
// the 2 P working blocks are co-resident exactly when 2 P <= CUs; refusal: the caller's message with (2 P, CUs).
template <size_t SMEM, class Args>
int launch_tower_update(void (*kern)(Args), const Args& a, hipStream_t stream, const char* what,
                        const char* refusal) {
    static_assert(SMEM <= 160 * 1024, "tower update LDS image exceeds 160 KiB");
    static_assert(SMEM > 80 * 1024, "one workgroup per CU: the residency argument needs > 80 KiB LDS");
    const int cus = device_cu_count();
    if (2 * a.P > cus) {
        set_error(refusal, 2 * a.P, cus);
        return PGM_E_UNSUPPORTED;
    }
    // norm granules + timeout word start at tag 0
    if (int rc = prepare_update_launch((const void*)kern, MT, SMEM, 2 * a.P, a.ws, ppo_flag_bytes(a.P), stream, what))
        return rc;
    hipLaunchKernelGGL(kern, dim3(tower_grid(a.P)), dim3(MT), SMEM, stream, a);
    return launch_status(what);
}

}  // namespace pgm
