// cbhg.h — what cbhg.hip shares with its C-ABI host file (capi_cbhg.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace wrnn {
namespace cbhg {

constexpr int kC = 128;          // channels of the bank, the highways and one GRU direction
constexpr int kGates = 3 * kC;   // r, z, n rows of one direction
constexpr int kTilePos = 32;     // positions per workgroup of the position kernels
constexpr int kTileOut = 128;    // outputs per workgroup
constexpr int kChunk = 128;      // input channels staged in LDS at a time
constexpr int kMaxTaps = 16;
constexpr int kThreads = 256;

// One weight tensor's way into the packed block: a conv / linear weight [O][cin][taps] (PyTorch
// layout) goes to dst[(j·cin + c)·ld + col0 + o]; a vector is O = n, cin = taps = 1, ld = n.
struct Repack {
    const float *src;
    int64_t dst;     // floats from the packed block's start
    int32_t O, cin, taps, ld, col0, pad_;
};

enum Epilogue { kLinear = 0, kRelu = 1, kReluBn = 2, kBnResidual = 3 };

// out[p][col0 + o] = epilogue(bias[o] + Σ_chunk Σ_j Σ_c wt[(j·cin + c)·O + o] · x[row(p + j − taps/2)][c]),
// taps outside the position's own sentence selected away.  bank != 0: blockIdx.z + 1 is the tap count.
struct Gemm {
    const float *x;
    const int32_t *gather;   // row(q) = gather[q] when set (the embedding lookup), else q
    int32_t ldx, cin, taps;
    const float *wt;
    int32_t O;
    float *out;
    int32_t ldo, col0, mode;
    const float *bias;       // [O] or null
    const float *bn;         // [4][O]: weight, bias, running_mean, running_var
    const float *res;        // [P][ldres], mode kBnResidual
    int32_t ldres;
    const int32_t *bounds;   // [P][2]: first and one-past-last position of the position's sentence
    int32_t P, bank;
};

hipError_t launch_repack(const Repack *table, int n, float *packed, hipStream_t st);
hipError_t launch_gemm(const Gemm &g, hipStream_t st);
hipError_t launch_pool(const float *bank, float *pooled, int width, const int32_t *bounds, int P, hipStream_t st);
// y = g·relu(a) + (1 − g)·x with a = t[p][0..127], g = sigmoid(t[p][128..255])
hipError_t launch_highway(const float *t, const float *x, float *y, int P, hipStream_t st);
// gi [P][768] (forward r z n, backward r z n, b_ih included); whh_* [384][128] in place; bhh [2][384]
hipError_t launch_gru_scan(const float *gi, const float *whh_f, const float *whh_b, const float *bhh, float *out,
                           const int32_t *order, const int32_t *offsets, int n_seq, hipStream_t st);

}  // namespace cbhg
}  // namespace wrnn
