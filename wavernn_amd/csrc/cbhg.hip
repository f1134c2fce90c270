// cbhg.hip — the Tacotron CBHGs (encoder, postnet) for N sentences of N lengths packed on the time
// axis.  Every stage is its own launch on the caller's stream; no workgroup waits
// for another.  fp32 throughout, plain FMAs: every output value is ONE accumulator summed in an
// order the layer's shape fixes (channel chunk, tap, channel), so it cannot depend on the number of
// sentences, on the slot, on the neighbours or on where a tile starts.  Positions outside a
// sentence are selected away (never multiplied by zero), so a NaN stays in its own sentence.
#include <hip/hip_runtime.h>

#include "cbhg.h"

namespace wrnn {
namespace cbhg {

// ---------------------------------------------------------------- weights → [tap][channel][output]
__global__ __launch_bounds__(kThreads) void repack_kernel(const Repack *table, float *packed) {
    const Repack d = table[blockIdx.y];
    const int64_t n = (int64_t)d.O * d.cin * d.taps;
    float *dst = packed + d.dst;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const int o = (int)(e % d.O);
        const int64_t jc = e / d.O;
        const int c = (int)(jc % d.cin), j = (int)(jc / d.cin);
        dst[jc * d.ld + d.col0 + o] = d.src[((int64_t)o * d.cin + c) * d.taps + j];
    }
}

hipError_t launch_repack(const Repack *table, int n, float *packed, hipStream_t st) {
    hipLaunchKernelGGL(repack_kernel, dim3(64, n), dim3(kThreads), 0, st, table, packed);
    return hipGetLastError();
}

// ---------------------------------------------------------------- positions × (taps · channels) → outputs
constexpr int kRowLd = kChunk + 4;                       // LDS row stride: 16-byte rows, off the bank period
constexpr int kRowsMax = kTilePos + kMaxTaps - 1;

__device__ __forceinline__ float4 sel4(bool v, float4 a) { return v ? a : make_float4(0.f, 0.f, 0.f, 0.f); }

__global__ __launch_bounds__(kThreads) void gemm_kernel(const Gemm g) {
    __shared__ __attribute__((aligned(16))) float xs[kRowsMax * kRowLd];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int taps = g.bank ? (int)blockIdx.z + 1 : g.taps;
    const int pad = taps / 2;
    const int64_t wt_off = g.bank ? (int64_t)g.cin * g.O * ((int64_t)blockIdx.z * (blockIdx.z + 1) / 2) : 0;
    const float *wt = g.wt + wt_off;
    const int col0 = g.bank ? (int)blockIdx.z * g.O : g.col0;
    const float *bn = g.bn ? g.bn + (g.bank ? (int64_t)blockIdx.z * 4 * g.O : 0) : nullptr;
    const int p0 = blockIdx.x * kTilePos;
    const int o = blockIdx.y * kTileOut + tx * 4;
    const bool live = o < g.O;
    int lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = p0 + ty * 4 + r;
        lo[r] = p < g.P ? g.bounds[2 * p] : 0;
        hi[r] = p < g.P ? g.bounds[2 * p + 1] : 0;
    }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][i] = 0.f;
    const int rows = kTilePos + taps - 1;
    for (int c0 = 0; c0 < g.cin; c0 += kChunk) {
        const int cc = min(kChunk, g.cin - c0), cc4 = cc >> 2;
        __syncthreads();
        for (int e = tid; e < rows * cc4; e += kThreads) {
            const int i = e / cc4, c = (e - i * cc4) * 4;
            const int q = p0 - pad + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q >= 0 && q < g.P) {
                const int64_t row = g.gather ? g.gather[q] : q;
                v = *reinterpret_cast<const float4 *>(g.x + row * g.ldx + c0 + c);
            }
            *reinterpret_cast<float4 *>(&xs[i * kRowLd + c]) = v;
        }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < taps; ++j) {
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = p0 + ty * 4 + r + j - pad;
                ok[r] = q >= lo[r] && q < hi[r];
            }
            if (!(ok[0] || ok[1] || ok[2] || ok[3])) continue;     // adds nothing: every term is selected away
            const float *wj = wt + ((int64_t)j * g.cin + c0) * g.O + o;
            const float *xj = &xs[(ty * 4 + j) * kRowLd];
#pragma unroll 2
            for (int c = 0; c < cc; c += 4) {
                float4 xv[4], wv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) xv[r] = sel4(ok[r], *reinterpret_cast<const float4 *>(xj + r * kRowLd + c));
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = *reinterpret_cast<const float4 *>(wj + (int64_t)(c + i) * g.O);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xr[4] = {xv[r].x, xv[r].y, xv[r].z, xv[r].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[r][0] = fmaf(xr[i], wv[i].x, acc[r][0]);
                        acc[r][1] = fmaf(xr[i], wv[i].y, acc[r][1]);
                        acc[r][2] = fmaf(xr[i], wv[i].z, acc[r][2]);
                        acc[r][3] = fmaf(xr[i], wv[i].w, acc[r][3]);
                    }
                }
            }
        }
    }
    if (!live) return;
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f), bw = bias, bb = bias, bm = bias, bv = bias;
    if (g.bias) bias = *reinterpret_cast<const float4 *>(g.bias + o);
    if (bn) {
        bw = *reinterpret_cast<const float4 *>(bn + o);
        bb = *reinterpret_cast<const float4 *>(bn + g.O + o);
        bm = *reinterpret_cast<const float4 *>(bn + 2 * g.O + o);
        bv = *reinterpret_cast<const float4 *>(bn + 3 * g.O + o);
    }
    const float b4[4] = {bias.x, bias.y, bias.z, bias.w}, w4[4] = {bw.x, bw.y, bw.z, bw.w}, s4[4] = {bb.x, bb.y, bb.z, bb.w},
                m4[4] = {bm.x, bm.y, bm.z, bm.w}, v4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = p0 + ty * 4 + r;
        if (p >= g.P) continue;
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = acc[r][i];
            if (g.bias) v += b4[i];
            if (g.mode == kRelu || g.mode == kReluBn) v = fmaxf(v, 0.f);
            if (g.mode == kReluBn || g.mode == kBnResidual) v = (v - m4[i]) / sqrtf(v4[i] + 1e-5f) * w4[i] + s4[i];
            y[i] = v;
        }
        if (g.mode == kBnResidual) {
            const float4 x = *reinterpret_cast<const float4 *>(g.res + (int64_t)p * g.ldres + o);
            y[0] += x.x, y[1] += x.y, y[2] += x.z, y[3] += x.w;
        }
        *reinterpret_cast<float4 *>(g.out + (int64_t)p * g.ldo + col0 + o) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

hipError_t launch_gemm(const Gemm &g, hipStream_t st) {
    const dim3 grid((g.P + kTilePos - 1) / kTilePos, (g.O + kTileOut - 1) / kTileOut, g.bank ? g.bank : 1);
    hipLaunchKernelGGL(gemm_kernel, grid, dim3(kThreads), 0, st, g);
    return hipGetLastError();
}

// ---------------------------------------------------------------- max-pool(2, stride 1, padding 1)[:T]
__global__ __launch_bounds__(kThreads) void pool_kernel(const float *bank, float *pooled, int w4, const int32_t *bounds,
                                                        int64_t n4) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n4; e += (int64_t)gridDim.x * kThreads) {
        const int p = (int)(e / w4);
        float4 v = reinterpret_cast<const float4 *>(bank)[e];
        if (p > bounds[2 * p]) {     // the sentence's first position has no left neighbour (−inf padding)
            const float4 l = reinterpret_cast<const float4 *>(bank)[e - w4];
            v = make_float4(fmaxf(l.x, v.x), fmaxf(l.y, v.y), fmaxf(l.z, v.z), fmaxf(l.w, v.w));
        }
        reinterpret_cast<float4 *>(pooled)[e] = v;
    }
}

hipError_t launch_pool(const float *bank, float *pooled, int width, const int32_t *bounds, int P, hipStream_t st) {
    const int64_t n4 = (int64_t)P * (width / 4);
    const int blocks = (int)((n4 + kThreads - 1) / kThreads < 4096 ? (n4 + kThreads - 1) / kThreads : 4096);
    hipLaunchKernelGGL(pool_kernel, dim3(blocks), dim3(kThreads), 0, st, bank, pooled, width / 4, bounds, n4);
    return hipGetLastError();
}

// ---------------------------------------------------------------- highway combine
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(kThreads) void highway_kernel(const float *t, const float *x, float *y, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t p = e / kC;
        const int c = (int)(e - p * kC);
        const float a = fmaxf(t[p * 2 * kC + c], 0.f), gate = sigmoidf_(t[p * 2 * kC + kC + c]);
        y[e] = gate * a + (1.f - gate) * x[e];
    }
}

hipError_t launch_highway(const float *t, const float *x, float *y, int P, hipStream_t st) {
    const int64_t n = (int64_t)P * kC;
    const int blocks = (int)((n + kThreads - 1) / kThreads < 4096 ? (n + kThreads - 1) / kThreads : 4096);
    hipLaunchKernelGGL(highway_kernel, dim3(blocks), dim3(kThreads), 0, st, t, x, y, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the bidirectional GRU's scan
// One workgroup per (sentence, direction), longest sentence first.  W_hh of the direction (384 × 128
// fp32 = 192 KB) lives in registers for the whole scan: thread (unit u = tid % 128, half = tid / 128)
// holds columns half·64 .. half·64 + 63 of unit u's r, z and n rows (192 VGPRs).  A step: every thread
// reads its 64 h values from LDS and sums its three partial dots; the upper half hands its partials
// over through LDS (barrier 1); the lower half adds them (lower + upper, then the bias), applies the
// gates, writes h to LDS and the output row (barrier 2).  The next step's gi values are loaded at the
// top of the step and arrive under the dots.
__global__ __launch_bounds__(kThreads) void gru_scan_kernel(const float *gi, const float *whh_f, const float *whh_b,
                                                            const float *bhh, float *out, const int32_t *order,
                                                            const int32_t *offsets) {
    __shared__ __attribute__((aligned(16))) float hs[kC];
    __shared__ float part[3][kC];
    const int tid = threadIdx.x, u = tid & (kC - 1), half = tid >> 7;
    const int s = order[blockIdx.x >> 1], dir = blockIdx.x & 1;
    const int t0 = offsets[s], T = offsets[s + 1] - t0;
    const float *W = dir ? whh_b : whh_f;
    float w[3][64];
#pragma unroll
    for (int gt = 0; gt < 3; ++gt)
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(W + (int64_t)(gt * kC + u) * kC + half * 64 + c);
            w[gt][c] = v.x, w[gt][c + 1] = v.y, w[gt][c + 2] = v.z, w[gt][c + 3] = v.w;
        }
    float bh[3] = {0.f, 0.f, 0.f};
    if (half == 0) {
#pragma unroll
        for (int gt = 0; gt < 3; ++gt) bh[gt] = bhh[dir * kGates + gt * kC + u];
        hs[u] = 0.f;
    }
    __syncthreads();
    const int step = dir ? -1 : 1;
    int pos = dir ? t0 + T - 1 : t0;
    const float *gp = gi + dir * kGates + u;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, h = 0.f;
    if (half == 0) {
        g0 = gp[(int64_t)pos * 2 * kGates], g1 = gp[(int64_t)pos * 2 * kGates + kC], g2 = gp[(int64_t)pos * 2 * kGates + 2 * kC];
    }
    for (int i = 0; i < T; ++i) {
        float n0 = 0.f, n1 = 0.f, n2 = 0.f;
        if (half == 0 && i + 1 < T) {
            const int64_t q = (int64_t)(pos + step) * 2 * kGates;
            n0 = gp[q], n1 = gp[q + kC], n2 = gp[q + 2 * kC];
        }
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            const float4 hv = *reinterpret_cast<const float4 *>(&hs[half * 64 + c]);
            const float h4[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0 = fmaf(w[0][c + k], h4[k], a0);
                a1 = fmaf(w[1][c + k], h4[k], a1);
                a2 = fmaf(w[2][c + k], h4[k], a2);
            }
        }
        if (half == 1) part[0][u] = a0, part[1][u] = a1, part[2][u] = a2;
        __syncthreads();
        if (half == 0) {
            a0 = (a0 + part[0][u]) + bh[0];
            a1 = (a1 + part[1][u]) + bh[1];
            a2 = (a2 + part[2][u]) + bh[2];
            const float r = sigmoidf_(g0 + a0), z = sigmoidf_(g1 + a1);
            const float n = tanhf(g2 + r * a2);
            h = (1.f - z) * n + z * h;
            hs[u] = h;
            out[(int64_t)pos * 2 * kC + dir * kC + u] = h;
        }
        __syncthreads();
        pos += step;
        g0 = n0, g1 = n1, g2 = n2;
    }
}

hipError_t launch_gru_scan(const float *gi, const float *whh_f, const float *whh_b, const float *bhh, float *out,
                           const int32_t *order, const int32_t *offsets, int n_seq, hipStream_t st) {
    hipLaunchKernelGGL(gru_scan_kernel, dim3(2 * n_seq), dim3(kThreads), 0, st, gi, whh_f, whh_b, bhh, out, order, offsets);
    return hipGetLastError();
}

}  // namespace cbhg
}  // namespace wrnn
