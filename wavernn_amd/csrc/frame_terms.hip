// frame_terms.hip — the persistent kernels' conditioning terms formed at FRAME rate.
//
// Every MoL / RAW persistent kernel reads, per loop row and step, terms = W·[mel_up(p) | aux(p) | 1]
// (the I layer of fatchord_version.py:201-206 folded with the input halves of both GRUs, fc1 and
// fc2 into one matrix W, capi.cpp).  The reference's UpsampleNetwork (:64-89) is linear and, in
// units of frames, shift-invariant: with f = p div hop and φ = p mod hop,
//   mel_up(p) = Σ_k coef[φ][k] · mel[f + k + jlo],   coef[φ][k] = κ(φ − hop·(k + jlo)),
// κ the Stretch2d/Conv2d cascade's response to one frame (the cascade's zero padding is the
// frame-level zero padding once pad_tensor's pad frames cover κ's reach), and aux(p) = aux[f]
// (resnet_stretch, :83).  Hence
//   terms(p) = Σ_k coef[φ][k] · FT[f + k] + AT[f],
//   FT[i] = W·[mel[i + jlo] | 0 | 0],   AT[f] = W·[0 | aux[f] | 1],   AT[n_frames] = W·[0 | 0 | 1]
// (the last row: steps past the utterance, fold_with_overlap's zero tail, :317-330).  The terms
// GEMM runs over the n_frames frames instead of the hop·n_frames samples (hop 275: 275× fewer
// flops); what is left per sample is this nJ-tap sum over cached rows, an HBM-write-bound pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fatchord_xcd.h"
#include "fatchord_xcdm.h"
#include "frame_terms.h"

namespace wrnn {

// Frame-level conditioning records [frames][U][CD] for the path's own GEMM-input packer
// (pack_cond_input_kernel): kind 0 → record i = [mel[:, i + jlo] (0 outside [0, NF)) | 0 …],
// kind 1 → record f = [0 … | aux[:, f]] (f == NF: all zero).  mel [U][feat][NF], aux [U][A4][NF].
__global__ void frame_cond_kernel(const float *__restrict__ mel, const float *__restrict__ aux, int U, int feat, int A4,
                                  int NF, int frames, int jlo, int kind, float *__restrict__ rec) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);   // record (frame · U + u), one wave each
    if (m >= frames * U) return;
    const int i = m / U, u = m - i * U;
    const int CD = feat + A4;
    float *dst = rec + (size_t)m * CD;
    for (int c = threadIdx.x & 63; c < CD; c += 64) {
        float v = 0.0f;
        if (kind == 0) {
            const int fr = i + jlo;
            if (c < feat && fr >= 0 && fr < NF) v = mel[((size_t)u * feat + c) * NF + fr];
        } else if (c >= feat && i < NF) {
            v = aux[((size_t)u * A4 + (c - feat)) * NF + i];
        }
        dst[c] = v;
    }
}

hipError_t launch_frame_cond(const float *mel, const float *aux, int U, int feat, int A4, int NF, int frames, int jlo,
                             int kind, float *rec, hipStream_t st) {
    const int M = frames * U;
    hipLaunchKernelGGL(frame_cond_kernel, dim3((M + 3) / 4), dim3(256), 0, st, mel, aux, U, feat, A4, NF, frames, jlo,
                       kind, rec);
    return hipGetLastError();
}

struct InterpArgs {
    const float *FT;      // [NFF][U][N]   W·(one mel frame)
    const float *AT;      // [NF + 1][U][N] W·(aux frame, ones); row NF: W·(ones)
    const float *coef;    // [hop][nJ]
    float *T;             // [nt · nb][N]  record (t − t0)·nb + k
    int N, U, NF, NFF, hop, nJ;
    int nf, stride;       // loop row r: utterance r / nf, first step (r % nf)·stride
    int b0, nb, t0, nt;
};

constexpr int kInterpThreads = 256;
constexpr int kInterpSteps = 32;   // consecutive steps of one row per workgroup: a frame's rows (hop ≥ 32
                                   // steps) are loaded once and stay in registers
constexpr int kInterpMaxJ = 8;

// One workgroup: a 1 024-float column slice (a float4 per lane) of kInterpSteps consecutive steps of
// ONE loop row.  The frame rows FT[f .. f + nJ) and AT[f] are reloaded only when the step crosses
// into another frame (wave-uniform branch), so the pass reads ≈ 6/32 of what it writes: it is
// bound by the terms it writes, not by re-reading cached rows (8 records of 8 rows per workgroup
// reloaded all six rows per record: 2.2 TB/s effective).
__global__ __launch_bounds__(kInterpThreads) void terms_interp_kernel(InterpArgs a) {
    const int c4 = blockIdx.y * kInterpThreads + threadIdx.x;   // float4 column
    if (4 * c4 >= a.N) return;
    const int nblk = (a.nt + kInterpSteps - 1) / kInterpSteps;
    const int k = blockIdx.x / nblk, tb = (blockIdx.x - k * nblk) * kInterpSteps;
    const int r = a.b0 + k, u = r / a.nf;
    const int s0 = (r - u * a.nf) * a.stride + a.t0;            // utterance position of step t0
    const int L_utt = a.NF * a.hop;
    const size_t rs = (size_t)a.U * a.N;                         // frame-row stride
    const float *A0 = a.AT + (size_t)u * a.N + 4 * c4, *F0 = a.FT + (size_t)u * a.N + 4 * c4;
    float4 fr[kInterpMaxJ], ar = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int loaded = -1;
    for (int i = 0; i < kInterpSteps; ++i) {
        const int tl = tb + i;
        if (tl >= a.nt) break;
        const int p = s0 + tl;
        const int f = p < L_utt ? p / a.hop : a.NF;               // a.NF: past the utterance (W·[0 | 0 | 1])
        if (f != loaded) {
            ar = *reinterpret_cast<const float4 *>(A0 + (size_t)f * rs);
            if (f < a.NF) {
#pragma unroll
                for (int j = 0; j < kInterpMaxJ; ++j)
                    if (j < a.nJ) fr[j] = *reinterpret_cast<const float4 *>(F0 + (size_t)(f + j) * rs);
            }
            loaded = f;
        }
        float4 acc = ar;
        if (f < a.NF) {
            const float *cf = a.coef + (size_t)(p - f * a.hop) * a.nJ;
#pragma unroll
            for (int j = 0; j < kInterpMaxJ; ++j) {
                if (j < a.nJ) {
                    const float w = cf[j];
                    acc.x = fmaf(w, fr[j].x, acc.x);
                    acc.y = fmaf(w, fr[j].y, acc.y);
                    acc.z = fmaf(w, fr[j].z, acc.z);
                    acc.w = fmaf(w, fr[j].w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4 *>(a.T + ((size_t)tl * a.nb + k) * a.N + 4 * c4) = acc;
    }
}

// N % 4 == 0 and nJ <= kInterpMaxJ (the host checks both before choosing the frame path)
hipError_t launch_terms_interp(const float *FT, const float *AT, const float *coef, float *T, int N, int U, int NF,
                               int NFF, int hop, int nJ, int nf, int stride, int b0, int nb, int t0, int nt,
                               hipStream_t st) {
    InterpArgs a{FT, AT, coef, T, N, U, NF, NFF, hop, nJ, nf, stride, b0, nb, t0, nt};
    const dim3 grid(nb * ((nt + kInterpSteps - 1) / kInterpSteps), (N / 4 + kInterpThreads - 1) / kInterpThreads);
    hipLaunchKernelGGL(terms_interp_kernel, grid, dim3(kInterpThreads), 0, st, a);
    return hipGetLastError();
}

// ---- streaming sessions (wrnn_stream_*): the same pass over a WINDOW of frame rows ---------------
// A session appends FT / AT rows as mel frames arrive and drops the rows behind the loop, so the
// stores hold rows [ft_base, …) / [at_base, …) of the absolute numbering above (FT row i = mel frame
// i + jlo, AT row f = aux frame f).  Loop row k is utterance k (unbatched: nf = 1), and an unbatched
// loop has no step past its utterance (the last launch forms no terms row beyond step T·hop − 1),
// so neither the frame count nor a W·[0 | 0 | 1] row enters: every step reads its own frame's rows.
// The per-sample fmaf order is terms_interp_kernel's.
struct InterpWinArgs {
    const float *FT;      // [rows][U][N], row 0 = absolute row ft_base
    const float *AT;      // [rows][U][N], row 0 = absolute row at_base
    const float *coef;    // [hop][nJ]
    float *T;             // [nt · nb][N]  record (t − t0)·nb + k
    int N, U, hop, nJ;
    int ft_base, at_base;
    int nb, t0, nt;
};

__global__ __launch_bounds__(kInterpThreads) void terms_interp_win_kernel(InterpWinArgs a) {
    const int c4 = blockIdx.y * kInterpThreads + threadIdx.x;   // float4 column
    if (4 * c4 >= a.N) return;
    const int nblk = (a.nt + kInterpSteps - 1) / kInterpSteps;
    const int k = blockIdx.x / nblk, tb = (blockIdx.x - k * nblk) * kInterpSteps;
    const size_t rs = (size_t)a.U * a.N;                         // frame-row stride
    const float *A0 = a.AT + (size_t)k * a.N + 4 * c4, *F0 = a.FT + (size_t)k * a.N + 4 * c4;
    float4 fr[kInterpMaxJ], ar = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int loaded = -1;
    for (int i = 0; i < kInterpSteps; ++i) {
        const int tl = tb + i;
        if (tl >= a.nt) break;
        const int p = a.t0 + tl;
        const int f = p / a.hop;
        if (f != loaded) {
            ar = *reinterpret_cast<const float4 *>(A0 + (size_t)(f - a.at_base) * rs);
#pragma unroll
            for (int j = 0; j < kInterpMaxJ; ++j)
                if (j < a.nJ) fr[j] = *reinterpret_cast<const float4 *>(F0 + (size_t)(f + j - a.ft_base) * rs);
            loaded = f;
        }
        float4 acc = ar;
        const float *cf = a.coef + (size_t)(p - f * a.hop) * a.nJ;
#pragma unroll
        for (int j = 0; j < kInterpMaxJ; ++j) {
            if (j < a.nJ) {
                const float w = cf[j];
                acc.x = fmaf(w, fr[j].x, acc.x);
                acc.y = fmaf(w, fr[j].y, acc.y);
                acc.z = fmaf(w, fr[j].z, acc.z);
                acc.w = fmaf(w, fr[j].w, acc.w);
            }
        }
        *reinterpret_cast<float4 *>(a.T + ((size_t)tl * a.nb + k) * a.N + 4 * c4) = acc;
    }
}

// The caller holds FT rows [t0 / hop, (t0 + nt − 1) / hop + nJ) and AT rows [t0 / hop, (t0 + nt − 1) / hop]
// in its stores; N % 4 == 0, nJ <= kInterpMaxJ, nb == U.
hipError_t launch_terms_interp_win(const float *FT, int ft_base, const float *AT, int at_base, const float *coef,
                                   float *T, int N, int U, int hop, int nJ, int t0, int nt, hipStream_t st) {
    InterpWinArgs a{FT, AT, coef, T, N, U, hop, nJ, ft_base, at_base, U, t0, nt};
    const dim3 grid(U * ((nt + kInterpSteps - 1) / kInterpSteps), (N / 4 + kInterpThreads - 1) / kInterpThreads);
    hipLaunchKernelGGL(terms_interp_win_kernel, grid, dim3(kInterpThreads), 0, st, a);
    return hipGetLastError();
}

// ---- wide streaming groups (capi_stream.cpp: wide_group_launches): the windowed pass for every row of one
// launch, from the row table (fatchord_xcdm.h: XcdmRow) — row k's frame-term stores, their bases and
// its first step — into column k of the launch-shared record [nt][nb][N].  The stores are in the
// many-row kernel's segmented record order already (the pass is elementwise); per sample the sum
// runs in terms_interp_kernel's order.
__global__ __launch_bounds__(kInterpThreads) void terms_interp_wide_kernel(const XcdmRow *rows, const float *coef,
                                                                            float *T, int N, int hop, int nJ, int nb,
                                                                            int nt) {
    const int c4 = blockIdx.y * kInterpThreads + threadIdx.x;   // float4 column
    if (4 * c4 >= N) return;
    const int nblk = (nt + kInterpSteps - 1) / kInterpSteps;
    const int k = blockIdx.x / nblk, tb = (blockIdx.x - k * nblk) * kInterpSteps;
    const XcdmRow &r = rows[k];
    const size_t rs = (size_t)r.fr_ld;                          // frame-row stride
    const float *A0 = r.at + 4 * c4, *F0 = r.ft + 4 * c4;
    float4 fr[kInterpMaxJ], ar = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int loaded = -1;
    for (int i = 0; i < kInterpSteps; ++i) {
        const int tl = tb + i;
        if (tl >= nt) break;
        const int p = r.t0 + tl;
        const int f = p / hop;
        if (f != loaded) {
            ar = *reinterpret_cast<const float4 *>(A0 + (size_t)(f - r.at_base) * rs);
#pragma unroll
            for (int j = 0; j < kInterpMaxJ; ++j)
                if (j < nJ) fr[j] = *reinterpret_cast<const float4 *>(F0 + (size_t)(f + j - r.ft_base) * rs);
            loaded = f;
        }
        float4 acc = ar;
        const float *cf = coef + (size_t)(p - f * hop) * nJ;
#pragma unroll
        for (int j = 0; j < kInterpMaxJ; ++j) {
            if (j < nJ) {
                const float w = cf[j];
                acc.x = fmaf(w, fr[j].x, acc.x);
                acc.y = fmaf(w, fr[j].y, acc.y);
                acc.z = fmaf(w, fr[j].z, acc.z);
                acc.w = fmaf(w, fr[j].w, acc.w);
            }
        }
        *reinterpret_cast<float4 *>(T + ((size_t)tl * nb + k) * N + 4 * c4) = acc;
    }
}

// Every row's stores hold the FT / AT rows of its steps [t0, t0 + nt); N % 4 == 0, nJ <= kInterpMaxJ
hipError_t launch_terms_interp_wide(const XcdmRow *rows, const float *coef, float *T, int N, int hop, int nJ, int nb,
                                    int nt, hipStream_t st) {
    const dim3 grid(nb * ((nt + kInterpSteps - 1) / kInterpSteps), (N / 4 + kInterpThreads - 1) / kInterpThreads);
    hipLaunchKernelGGL(terms_interp_wide_kernel, grid, dim3(kInterpThreads), 0, st, rows, coef, T, N, hop, nJ, nb, nt);
    return hipGetLastError();
}

// ---- folded lists (capi_lists.cpp: wrnn_generate_list_folds): the table-driven pass for fold rows --------
// Launch row k is one fold of some utterance: its XcdmRow gives the utterance's whole frame-term
// stores (base 0, fr_ld floats between frame rows), its FoldRow the utterance position of launch
// step 0 and the utterance's frame count.  A fold may start inside a frame (target + overlap need
// not be a multiple of hop) and its last steps may lie past the utterance: from position hop·NF on
// the terms are the row AT[NF] = W·[0 | 0 | 1] alone and no FT row is read, exactly as
// terms_interp_kernel does it.  Per sample the fmaf order is terms_interp_kernel's, so a fold row's
// terms are the bits wrnn_generate_frames forms for the same fold.
__global__ __launch_bounds__(kInterpThreads) void terms_interp_folds_kernel(const XcdmRow *rows, const FoldRow *folds,
                                                                             const float *coef, float *T, int N, int hop,
                                                                             int nJ, int nb, int nt) {
    const int c4 = blockIdx.y * kInterpThreads + threadIdx.x;   // float4 column
    if (4 * c4 >= N) return;
    const int nblk = (nt + kInterpSteps - 1) / kInterpSteps;
    const int k = blockIdx.x / nblk, tb = (blockIdx.x - k * nblk) * kInterpSteps;
    const XcdmRow &r = rows[k];
    const int NF = folds[k].NF;
    const int s0 = folds[k].pos0, L_utt = NF * hop;           // the plan keeps every position below 2^31
    const size_t rs = (size_t)r.fr_ld;                          // frame-row stride
    const float *A0 = r.at + 4 * c4, *F0 = r.ft + 4 * c4;
    float4 fr[kInterpMaxJ], ar = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int loaded = -1;
    for (int i = 0; i < kInterpSteps; ++i) {
        const int tl = tb + i;
        if (tl >= nt) break;
        const int p = s0 + tl;
        const int f = p < L_utt ? p / hop : NF;                 // NF: past the utterance (W·[0 | 0 | 1])
        if (f != loaded) {
            ar = *reinterpret_cast<const float4 *>(A0 + (size_t)f * rs);
            if (f < NF) {
#pragma unroll
                for (int j = 0; j < kInterpMaxJ; ++j)
                    if (j < nJ) fr[j] = *reinterpret_cast<const float4 *>(F0 + (size_t)(f + j) * rs);
            }
            loaded = f;
        }
        float4 acc = ar;
        if (f < NF) {
            const float *cf = coef + (size_t)(p - f * hop) * nJ;
#pragma unroll
            for (int j = 0; j < kInterpMaxJ; ++j) {
                if (j < nJ) {
                    const float w = cf[j];
                    acc.x = fmaf(w, fr[j].x, acc.x);
                    acc.y = fmaf(w, fr[j].y, acc.y);
                    acc.z = fmaf(w, fr[j].z, acc.z);
                    acc.w = fmaf(w, fr[j].w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4 *>(T + ((size_t)tl * nb + k) * N + 4 * c4) = acc;
    }
}

// Every row's stores hold FT rows [0, NF + nJ − 1) and AT rows [0, NF]; N % 4 == 0, nJ <= kInterpMaxJ
hipError_t launch_terms_interp_folds(const XcdmRow *rows, const FoldRow *folds, const float *coef, float *T, int N,
                                     int hop, int nJ, int nb, int nt, hipStream_t st) {
    const dim3 grid(nb * ((nt + kInterpSteps - 1) / kInterpSteps), (N / 4 + kInterpThreads - 1) / kInterpThreads);
    hipLaunchKernelGGL(terms_interp_folds_kernel, grid, dim3(kInterpThreads), 0, st, rows, folds, coef, T, N, hop, nJ, nb,
                       nt);
    return hipGetLastError();
}

// ---- list launches (wrnn_generate_list): the same pass for every piece of one round -------------
// Pieces p0 .. p1 − 1 of the device piece table (fatchord_xcd.h: XcdPiece) are the round's; piece p
// is steps [r.t0, r.t0 + nt) of one unbatched utterance (U = 1, nf = 1: the frame-row stride is N),
// its terms rows contiguous at r.terms, its frame rows at ft / at.  A step of an unbatched loop
// lies inside its utterance, and for a given (utterance, step) the sum runs in
// terms_interp_kernel's order: acc = AT[f], then fmaf(coef[φ][j], FT[f + j], acc) for j = 0 .. nJ − 1.
// blockIdx.x counts the kInterpSteps-step blocks of the pieces in table order (piece p: from blk0 on).
struct InterpListArgs {
    const XcdPiece *pieces;
    const float *coef;    // [hop][nJ]
    int p0, p1;
    int N, hop, nJ;
};

__global__ __launch_bounds__(kInterpThreads) void terms_interp_list_kernel(InterpListArgs a) {
    const int c4 = blockIdx.y * kInterpThreads + threadIdx.x;   // float4 column
    if (4 * c4 >= a.N) return;
    // the piece of this block: the last one whose first block (blk0, written by the host) is not past it
    int lo = a.p0, hi = a.p1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.pieces[mid].blk0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const int p = lo, blk = (int)blockIdx.x - a.pieces[p].blk0;
    if (blk * kInterpSteps >= a.pieces[p].nt) return;
    const XcdPiece &pc = a.pieces[p];
    const int nt = pc.nt, NF = pc.frames, s0 = pc.r.t0, tb = blk * kInterpSteps;
    const int L_utt = NF * a.hop;
    const size_t rs = (size_t)a.N;                               // frame-row stride (one utterance)
    const float *A0 = pc.at + 4 * c4, *F0 = pc.ft + 4 * c4;
    float *T = const_cast<float *>(pc.r.terms);
    float4 fr[kInterpMaxJ], ar = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int loaded = -1;
    for (int i = 0; i < kInterpSteps; ++i) {
        const int tl = tb + i;
        if (tl >= nt) break;
        const int ps = s0 + tl;
        const int f = ps < L_utt ? ps / a.hop : NF;
        if (f != loaded) {
            ar = *reinterpret_cast<const float4 *>(A0 + (size_t)f * rs);
            if (f < NF) {
#pragma unroll
                for (int j = 0; j < kInterpMaxJ; ++j)
                    if (j < a.nJ) fr[j] = *reinterpret_cast<const float4 *>(F0 + (size_t)(f + j) * rs);
            }
            loaded = f;
        }
        float4 acc = ar;
        if (f < NF) {
            const float *cf = a.coef + (size_t)(ps - f * a.hop) * a.nJ;
#pragma unroll
            for (int j = 0; j < kInterpMaxJ; ++j) {
                if (j < a.nJ) {
                    const float w = cf[j];
                    acc.x = fmaf(w, fr[j].x, acc.x);
                    acc.y = fmaf(w, fr[j].y, acc.y);
                    acc.z = fmaf(w, fr[j].z, acc.z);
                    acc.w = fmaf(w, fr[j].w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4 *>(T + (size_t)tl * a.N + 4 * c4) = acc;
    }
}

// `blocks` = Σ ⌈nt_p / kInterpSteps⌉ over the round's pieces (the host knows every nt);
// N % 4 == 0 and nJ <= kInterpMaxJ as above
hipError_t launch_terms_interp_list(const XcdPiece *pieces, int p0, int p1, int blocks, const float *coef, int N, int hop,
                                    int nJ, hipStream_t st) {
    if (blocks <= 0) return hipSuccess;
    InterpListArgs a{pieces, coef, p0, p1, N, hop, nJ};
    const dim3 grid(blocks, (N / 4 + kInterpThreads - 1) / kInterpThreads);
    hipLaunchKernelGGL(terms_interp_list_kernel, grid, dim3(kInterpThreads), 0, st, a);
    return hipGetLastError();
}

int interp_list_blocks(int nt) { return (nt + kInterpSteps - 1) / kInterpSteps; }

// The MelResNet input of a session's newly computable aux frames, and its carried mel tail, in one
// pass.  Frame g of the running mel is 0 outside [0, R_old + n) (pad_tensor's zeros: before the
// first frame and, once the end is known, after the last), chunk[:, g − R_old] for the frames of
// this push and tail_old[g − (R_old − keep)] for the `keep` frames before it.
//   chunk [U][feat][n], tail_old / tail_new [keep][U][feat], win [U][feat][wn] = frames w0 .. w0 + wn − 1,
//   tail_new = frames R_old + n − keep .. R_old + n − 1
__global__ void stream_mel_window_kernel(const float *__restrict__ tail_old, const float *__restrict__ chunk, int U,
                                         int feat, int n, int R_old, int keep, int w0, int wn,
                                         float *__restrict__ win, float *__restrict__ tail_new) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int W = wn + keep;
    if (idx >= U * feat * W) return;
    const int j = idx % W, uc = idx / W, c = uc % feat, u = uc / feat;
    const int g = j < wn ? w0 + j : R_old + n - keep + (j - wn);
    float v = 0.0f;
    if (g >= R_old && g < R_old + n) v = chunk[((size_t)u * feat + c) * n + (g - R_old)];
    else if (g >= 0 && g >= R_old - keep && g < R_old) v = tail_old[((size_t)(g - (R_old - keep)) * U + u) * feat + c];
    if (j < wn) win[((size_t)u * feat + c) * wn + j] = v;
    else tail_new[((size_t)(j - wn) * U + u) * feat + c] = v;
}

hipError_t launch_stream_mel_window(const float *tail_old, const float *chunk, int U, int feat, int n, int R_old,
                                    int keep, int w0, int wn, float *win, float *tail_new, hipStream_t st) {
    const int total = U * feat * (wn + keep);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_mel_window_kernel, dim3((total + 255) / 256), dim3(256), 0, st, tail_old, chunk, U, feat,
                       n, R_old, keep, w0, wn, win, tail_new);
    return hipGetLastError();
}

}  // namespace wrnn
