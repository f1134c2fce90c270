// tacotron_decoder.hip — the Tacotron decoder loop (prenet, attention GRU, location-sensitive
// attention, two residual LSTM cells, mel projection, stop test) for up to 128 sentences in ONE
// persistent launch.
//
// Partition.  One 256-thread workgroup per CU, grid G (256 on an MI355X).  Every output row of the
// big matrices belongs to one workgroup for the whole launch: workgroup w owns attention-GRU unit w,
// rnn_input outputs 2w and 2w+1, LSTM units 2w and 2w+1 of both cells (8 gate rows each) and a slice
// of mel_proj.  The per-sentence parts (prenet, the whole attention, the stop test) belong to the
// sentence's owner workgroup.  A step is seven phases with a grid barrier after each; activations
// cross workgroups through a small global scratch, the weights are read in place from the module's
// own fp32 tensors (each workgroup re-reads the same ~84 KB every step, which stays in its XCD's L2).
//
// Arithmetic.  Every dot product is computed by 32 lanes: lane l sums k = l, l+32, ... in order with
// fmaf, then a 5-stage xor butterfly.  The order depends on nothing but K, so a sentence's numbers
// do not depend on how many other sentences share the launch, nor on its slot.
#include <hip/hip_runtime.h>

#include "tacotron_decoder.h"

namespace wrnn {
namespace taco {

__device__ __forceinline__ float red32(float s) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}
__device__ __forceinline__ float red64(float s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// lane's share of a weight row: wr[i] = w[l + 32 i]
template <int K>
__device__ __forceinline__ void load_w(float (&wr)[(K + 31) / 32], const float *w, int l) {
#pragma unroll
    for (int i = 0; i < (K + 31) / 32; ++i) wr[i] = (l + 32 * i < K) ? w[l + 32 * i] : 0.0f;
}
template <int K>
__device__ __forceinline__ float acc_w(const float (&wr)[(K + 31) / 32], const float *x, int l, float s) {
#pragma unroll
    for (int i = 0; i < (K + 31) / 32; ++i)
        if (l + 32 * i < K) s = fmaf(wr[i], x[l + 32 * i], s);
    return s;
}

// Dot products of one weight row (two parts, wa over xa(b) and wb over xb(b)) with the rows
// act[first], act[first + stride], ...: four rows in flight per pass for latency, each with its own
// accumulator, so a row's summation order is what acc_w alone would give it.
template <int KA, int KB, class XA, class XB, class OUT>
__device__ __forceinline__ void rows_dot(const float (&wa)[(KA + 31) / 32], const float (&wb)[(KB + 31) / 32], int l, int first,
                                         int stride, int nact, const int *act, XA xa, XB xb, OUT out) {
    for (int i = first; i < nact; i += 4 * stride) {
        int idx[4], b[4];
        float s[4];
        const float *pa[4], *pb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            idx[j] = (i + j * stride < nact) ? i + j * stride : i;
            b[j] = act[idx[j]];
            pa[j] = xa(b[j]);
            pb[j] = xb(b[j]);
            s[j] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < (KA + 31) / 32; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = fmaf(wa[k], pa[j][l + 32 * k], s[j]);
#pragma unroll
        for (int k = 0; k < (KB + 31) / 32; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = fmaf(wb[k], pb[j][l + 32 * k], s[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = red32(s[j]);
            if (l == 0 && (j == 0 || i + j * stride < nact)) out(idx[j], b[j], s[j]);
        }
    }
}

struct Shared {
    int act[kMaxRows];
    int nact;
    int abort_;
    float gpre[kMaxRows][8];
    float cw[kF * 2 * kTaps];
    float cv[32][kF + 1];
    float win[2][32 + kTaps - 1];
    float part[32][4];
    float q[kD];
    float hq[kD];
    float f[kM];
    float a[kP1];
    float red[4];
};

// Grid barrier on one monotonic counter: plain stores drained by every wave, workgroup barrier,
// lane 0 releases at agent scope, adds, polls with relaxed agent loads (bounded by wall time),
// acquires; the workgroup barrier behind it holds the other waves until the invalidate is done.
__device__ __forceinline__ bool grid_barrier(unsigned *ctl, unsigned &epoch, int G, long long timeout, int step, int phase,
                                             Shared &sh) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    epoch += 1;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(ctl + kCounter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned want = epoch * (unsigned)G;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        unsigned spins = 0;
        for (;;) {
            const unsigned v = __hip_atomic_load(ctl + kCounter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v >= want) break;
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 63u) == 0) {
                const bool late = (long long)(__builtin_amdgcn_s_memrealtime() - t0) > timeout;
                const bool other = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                if (late || other) {
                    if (late && atomicCAS(ctl, 0u, 4u) == 0u) {
                        __hip_atomic_store(ctl + 1, (unsigned)step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(ctl + 2, (unsigned)phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(ctl + 3, (unsigned)blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    sh.abort_ = 1;
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    return sh.abort_ == 0;
}

// rows still to run: not stopped and below the step cap
__device__ __forceinline__ void list_active(const Args &a, Shared &sh) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int b = 0; b < a.rows; ++b) {
            const int *st = reinterpret_cast<const int *>(a.state + (size_t)b * a.state_ld);
            if (st[oSTOP] == 0 && st[oSTEP] < a.step_cap) sh.act[n++] = b;
        }
        sh.nact = n;
    }
    __syncthreads();
}

// prenet of the owner's row: fc1, ReLU, fc2, ReLU on the last frame
__device__ __forceinline__ void prenet(const Args &a, Shared &sh, int b) {
    const int tid = threadIdx.x, g = tid >> 5, l = tid & 31;
    const float *st = a.state + (size_t)b * a.state_ld;
    if (tid < kM) sh.f[tid] = st[oFRAME + tid];
    __syncthreads();
    for (int o = g * 32; o < g * 32 + 32; ++o) {
        float wr[3];
        load_w<kM>(wr, a.w.prenet_fc1_w + (size_t)o * kM, l);
        const float s = red32(acc_w<kM>(wr, sh.f, l, 0.0f));
        if (l == 0) sh.a[o] = fmaxf(s + a.w.prenet_fc1_b[o], 0.0f);
    }
    __syncthreads();
    float *p = a.scratch + kCtlWords + (size_t)b * kScratchRow + sP;
    for (int o = g * 16; o < g * 16 + 16; ++o) {
        float wr[8];
        load_w<kP1>(wr, a.w.prenet_fc2_w + (size_t)o * kP1, l);
        const float s = red32(acc_w<kP1>(wr, sh.a, l, 0.0f));
        if (l == 0) p[o] = fmaxf(s + a.w.prenet_fc2_b[o], 0.0f);
    }
}

// the whole location-sensitive attention of the owner's row at step s
__device__ __forceinline__ void attention(const Args &a, Shared &sh, int b, int s, const float (&Lr)[kF]) {
    const int tid = threadIdx.x, g = tid >> 5, l = tid & 31, wave = tid >> 6;
    const int T = a.t_enc[b];
    float *st = a.state + (size_t)b * a.state_ld;
    float *cum = st + oCUM, *att = st + oCUM + a.t_max;
    const float *hn = a.scratch + kCtlWords + (size_t)b * kScratchRow + sHN;
    float *out = a.attn + ((size_t)b * a.step_cap + s) * a.t_max;
    const float *proj = a.proj + (size_t)b * a.t_max * kD;
    const float *enc = a.enc + (size_t)b * a.t_max * kD;
    sh.hq[tid] = hn[tid];
    __syncthreads();
    for (int d = g * 32; d < g * 32 + 32; ++d) {
        float wr[8];
        load_w<kD>(wr, a.w.lsa_W_w + (size_t)d * kD, l);
        const float v = red32(acc_w<kD>(wr, sh.hq, l, 0.0f));
        if (l == 0) sh.q[d] = v + a.w.lsa_W_b[d];
    }
    const float Lb = a.w.lsa_L_b[tid], vd = a.w.lsa_v[tid];
    __syncthreads();
    const float qd = sh.q[tid];
    for (int t0 = 0; t0 < T; t0 += 32) {
        // the window of [cumulative, attention] this tile's taps touch, zero outside [0, T)
        if (tid < 2 * (32 + kTaps - 1)) {
            const int c = tid / (32 + kTaps - 1), i = tid % (32 + kTaps - 1);
            const int pos = t0 + i - (kTaps - 1) / 2;
            sh.win[c][i] = (pos >= 0 && pos < T) ? (c == 0 ? cum[pos] : att[pos]) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = tid + kThreads * j, tt = idx >> 5, f = idx & 31;
            float acc = 0.0f;
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < kTaps; ++k) acc = fmaf(sh.cw[(f * 2 + c) * kTaps + k], sh.win[c][tt + k], acc);
            sh.cv[tt][f] = acc;
        }
        __syncthreads();
        const int nt = min(32, T - t0);
        for (int tt = 0; tt < nt; ++tt) {
            float loc = Lb;
#pragma unroll
            for (int f = 0; f < kF; ++f) loc = fmaf(Lr[f], sh.cv[tt][f], loc);
            float e = vd * tanhf((qd + proj[(size_t)(t0 + tt) * kD + tid]) + loc);
            e = red64(e);
            if ((tid & 63) == 0) sh.part[tt][wave] = e;
        }
        __syncthreads();
        if (tid < nt) {
            const float u = ((sh.part[tid][0] + sh.part[tid][1]) + sh.part[tid][2]) + sh.part[tid][3];
            out[t0 + tid] = sigmoidf_(u);
        }
        __syncthreads();
    }
    // normaliser: strided partial sums, then a fixed tree (depends on T alone)
    float z = 0.0f;
    for (int t = tid; t < T; t += kThreads) z += out[t];
    z = red64(z);
    if ((tid & 63) == 0) sh.red[wave] = z;
    __syncthreads();
    const float Z = (sh.red[0] + sh.red[1]) + (sh.red[2] + sh.red[3]);
    for (int t = tid; t < T; t += kThreads) {
        const float sc = out[t] / Z;
        out[t] = sc;
        att[t] = sc;
        cum[t] += sc;
    }
    __syncthreads();
    float c = 0.0f;
    for (int t = 0; t < T; ++t) c = fmaf(att[t], enc[(size_t)t * kD + tid], c);
    st[oCTX + tid] = c;
}

__global__ __launch_bounds__(kThreads, 1) void decoder_loop(Args a) {
    __shared__ Shared sh;
    const int tid = threadIdx.x, g = tid >> 5, l = tid & 31;
    const int wg = blockIdx.x, G = gridDim.x;
    unsigned *ctl = reinterpret_cast<unsigned *>(a.scratch);
    float *sc = a.scratch + kCtlWords;
    unsigned epoch = 0;
    if (tid == 0) sh.abort_ = 0;
    int myrow = -1;
    for (int b = 0; b < a.rows; ++b)
        if ((b * G) / kMaxRows == wg) myrow = b;
    float Lr[kF];
#pragma unroll
    for (int f = 0; f < kF; ++f) Lr[f] = a.w.lsa_L_w[tid * kF + f];
    for (int i = tid; i < kF * 2 * kTaps; i += kThreads) sh.cw[i] = a.w.lsa_conv_w[i];
    const int r = a.r, nout = kM * r;

    list_active(a, sh);
    auto row_active = [&](int b) {
        const int *st = reinterpret_cast<const int *>(a.state + (size_t)b * a.state_ld);
        return st[oSTOP] == 0 && st[oSTEP] < a.step_cap;
    };
    if (sh.nact == 0 || a.n_steps <= 0) return;
    if (myrow >= 0 && row_active(myrow)) prenet(a, sh, myrow);
    if (!grid_barrier(ctl, epoch, G, a.timeout, 0, 0, sh)) return;

    for (int it = 0; it < a.n_steps; ++it) {
        const int nact = sh.nact;
        // ---- B: attention GRU cell on [context, prenet_out] --------------------------------------
        for (int u = wg; u < kD; u += G) {
            const int role = g & 3, half = g >> 2;
            const int gate = role < 2 ? role : 2;
            float wi_c[8], wi_p[4], wh[8];
            load_w<kD>(wi_c, a.w.attn_rnn_w_ih + (size_t)(gate * kD + u) * (kD + kP2), l);
            load_w<kP2>(wi_p, a.w.attn_rnn_w_ih + (size_t)(gate * kD + u) * (kD + kP2) + kD, l);
            load_w<kD>(wh, a.w.attn_rnn_w_hh + (size_t)(gate * kD + u) * kD, l);
            for (int i = half; i < nact; i += 2) {
                const int b = sh.act[i];
                const float *st = a.state + (size_t)b * a.state_ld;
                float s = 0.0f;
                if (role != 3) {
                    s = acc_w<kD>(wi_c, st + oCTX, l, s);
                    s = acc_w<kP2>(wi_p, sc + (size_t)b * kScratchRow + sP, l, s);
                }
                if (role == 3) s = acc_w<kD>(wh, st + oAH, l, s);
                s = red32(s);
                float s2 = 0.0f;
                if (role < 2) s2 = red32(acc_w<kD>(wh, st + oAH, l, 0.0f));
                if (l == 0) sh.gpre[i][role] = s + s2;
            }
            __syncthreads();
            if (tid < nact) {
                const int b = sh.act[tid];
                const float *bi = a.w.attn_rnn_b_ih, *bh = a.w.attn_rnn_b_hh;
                const float hp = a.state[(size_t)b * a.state_ld + oAH + u];
                const float rg = sigmoidf_((sh.gpre[tid][0] + bi[u]) + bh[u]);
                const float zg = sigmoidf_((sh.gpre[tid][1] + bi[kD + u]) + bh[kD + u]);
                const float ng = tanhf((sh.gpre[tid][2] + bi[2 * kD + u]) + rg * (sh.gpre[tid][3] + bh[2 * kD + u]));
                sc[(size_t)b * kScratchRow + sHN + u] = (1.0f - zg) * ng + zg * hp;
            }
            __syncthreads();
        }
        if (!grid_barrier(ctl, epoch, G, a.timeout, it, 1, sh)) return;

        // ---- C: location-sensitive attention and the context, by the row's owner ------------------
        if (myrow >= 0 && row_active(myrow)) {
            const int s = reinterpret_cast<const int *>(a.state + (size_t)myrow * a.state_ld)[oSTEP];
            attention(a, sh, myrow, s, Lr);
        }
        if (!grid_barrier(ctl, epoch, G, a.timeout, it, 2, sh)) return;

        // ---- D: rnn_input on [context, attn_hidden]; attn_hidden goes into the state ---------------
        for (int o0 = wg * 2; o0 < kH; o0 += G * 2) {
            const int o = o0 + (g & 1), part = g >> 1;
            float wc[8], wh[8];
            load_w<kD>(wc, a.w.rnn_input_w + (size_t)o * (2 * kD), l);
            load_w<kD>(wh, a.w.rnn_input_w + (size_t)o * (2 * kD) + kD, l);
            const float bias = a.w.rnn_input_b[o];
            rows_dot<kD, kD>(
                wc, wh, l, part, 4, nact, sh.act, [&](int b) { return a.state + (size_t)b * a.state_ld + oCTX; },
                [&](int b) { return sc + (size_t)b * kScratchRow + sHN; },
                [&](int, int b, float s) { sc[(size_t)b * kScratchRow + sX + o] = s + bias; });
        }
        for (int u = wg; u < kD; u += G)
            if (tid < nact) {
                const int b = sh.act[tid];
                a.state[(size_t)b * a.state_ld + oAH + u] = sc[(size_t)b * kScratchRow + sHN + u];
            }
        if (!grid_barrier(ctl, epoch, G, a.timeout, it, 3, sh)) return;

        // ---- E, F: the two residual LSTM cells ------------------------------------------------------
#pragma unroll 1
        for (int cell = 0; cell < 2; ++cell) {
            const float *wih = cell ? a.w.res_rnn2_w_ih : a.w.res_rnn1_w_ih, *whh = cell ? a.w.res_rnn2_w_hh : a.w.res_rnn1_w_hh;
            const float *bih = cell ? a.w.res_rnn2_b_ih : a.w.res_rnn1_b_ih, *bhh = cell ? a.w.res_rnn2_b_hh : a.w.res_rnn1_b_hh;
            const int sIn = cell ? sX1 : sX, sOut = cell ? sX2 : sX1, sHn = cell ? sH2N : sH1N;
            const int oHs = cell ? oH2 : oH1, oCs = cell ? oC2 : oC1;
            for (int j0 = wg * 2; j0 < kH; j0 += G * 2) {
                const int row = (g & 3) * kH + j0 + (g >> 2);
                float wx[16], wh[16];
                load_w<kH>(wx, wih + (size_t)row * kH, l);
                load_w<kH>(wh, whh + (size_t)row * kH, l);
                rows_dot<kH, kH>(
                    wx, wh, l, 0, 1, nact, sh.act, [&](int b) { return sc + (size_t)b * kScratchRow + sIn; },
                    [&](int b) { return a.state + (size_t)b * a.state_ld + oHs; },
                    [&](int i, int, float s) { sh.gpre[i][g] = s; });
                __syncthreads();
                if (tid < 2 * nact) {
                    const int i = tid >> 1, ju = tid & 1, j = j0 + ju, b = sh.act[i];
                    float *st = a.state + (size_t)b * a.state_ld;
                    const float gi = (sh.gpre[i][ju * 4 + 0] + bih[j]) + bhh[j];
                    const float gf = (sh.gpre[i][ju * 4 + 1] + bih[kH + j]) + bhh[kH + j];
                    const float gg = (sh.gpre[i][ju * 4 + 2] + bih[2 * kH + j]) + bhh[2 * kH + j];
                    const float go = (sh.gpre[i][ju * 4 + 3] + bih[3 * kH + j]) + bhh[3 * kH + j];
                    const float cn = sigmoidf_(gf) * st[oCs + j] + sigmoidf_(gi) * tanhf(gg);
                    const float hn = sigmoidf_(go) * tanhf(cn);
                    st[oCs + j] = cn;
                    sc[(size_t)b * kScratchRow + sHn + j] = hn;
                    sc[(size_t)b * kScratchRow + sOut + j] = sc[(size_t)b * kScratchRow + sIn + j] + hn;
                }
                __syncthreads();
                if (cell == 1 && tid < 2 * nact) {  // cell 1's new hidden, read by nobody any more
                    const int i = tid >> 1, j = j0 + (tid & 1), b = sh.act[i];
                    a.state[(size_t)b * a.state_ld + oH1 + j] = sc[(size_t)b * kScratchRow + sH1N + j];
                }
            }
            if (!grid_barrier(ctl, epoch, G, a.timeout, it, 4 + cell, sh)) return;
        }

        // ---- G: mel_proj rows mel*max_r + j, j < r; cell 2's new hidden goes into the state -----------
        {
            const int slots = 8 * G;
            int split = slots / nout;
            split = split < 1 ? 1 : (split > 8 ? 8 : split);
            for (int slot = wg + G * g; slot < nout * split; slot += slots) {
                const int qo = slot / split, part = slot % split;
                const int m = qo / r, j = qo % r;
                float wlo[8], whi[8];
                load_w<kD>(wlo, a.w.mel_proj_w + (size_t)(m * kMaxR + j) * kH, l);
                load_w<kD>(whi, a.w.mel_proj_w + (size_t)(m * kMaxR + j) * kH + kD, l);
                rows_dot<kD, kD>(
                    wlo, whi, l, part, split, nact, sh.act, [&](int b) { return sc + (size_t)b * kScratchRow + sX2; },
                    [&](int b) { return sc + (size_t)b * kScratchRow + sX2 + kD; },
                    [&](int, int b, float v) {
                        const int s = reinterpret_cast<const int *>(a.state + (size_t)b * a.state_ld)[oSTEP];
                        a.mel[((size_t)b * a.step_cap * r + (size_t)s * r + j) * kM + m] = v;
                    });
            }
            for (int j0 = wg * 2; j0 < kH; j0 += G * 2)
                if (tid < 2 * nact) {
                    const int i = tid >> 1, j = j0 + (tid & 1), b = sh.act[i];
                    a.state[(size_t)b * a.state_ld + oH2 + j] = sc[(size_t)b * kScratchRow + sH2N + j];
                }
        }
        if (!grid_barrier(ctl, epoch, G, a.timeout, it, 6, sh)) return;

        // ---- H + A: the stop test of this step and the next step's prenet, by the row's owner ----------
        if (myrow >= 0 && row_active(myrow)) {
            float *st = a.state + (size_t)myrow * a.state_ld;
            int *sti = reinterpret_cast<int *>(st);
            const int s = sti[oSTEP];
            const float *fr = a.mel + ((size_t)myrow * a.step_cap * r + (size_t)s * r) * kM;
            int loud = 0;
            for (int i = tid; i < nout; i += kThreads) loud |= !(fr[i] < a.thr);
            loud = __syncthreads_or(loud);
            const int stop = (!loud && s * r > 10) ? 1 : 0;
            if (tid < kM) st[oFRAME + tid] = fr[(r - 1) * kM + tid];
            __syncthreads();
            if (tid == 0) {
                sti[oSTEP] = s + 1;
                sti[oSTOP] = stop;
            }
            if (!stop && s + 1 < a.step_cap && it + 1 < a.n_steps) prenet(a, sh, myrow);
        }
        if (!grid_barrier(ctl, epoch, G, a.timeout, it, 7, sh)) return;
        list_active(a, sh);
        if (sh.nact == 0) return;
    }
}

hipError_t launch_decoder_loop(const Args &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(decoder_loop, dim3(grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace taco
}  // namespace wrnn
