// Shared between the host side (capi*.cpp) and fatchord_xcd.hip: the XCD-resident MoL
// kernel — one utterance (row) per XCD, its whole sample loop on that XCD's 32 CUs, every
// hand-off kept inside the XCD's L2.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace wrnn {

constexpr int kXcds = 8;            // XCDs of an MI355X (one row each)
constexpr int kXcdWgs = 32;         // workgroups (= CUs) per XCD, one per CU
constexpr int kXWaves = 8;          // waves per workgroup (two per SIMD), no loader wave
constexpr int kXThreads = 64 * kXWaves;
constexpr int kXUnits = 16;         // GRU units per workgroup (R / kXcdWgs), 4 per GRU2 wave
constexpr int kXFcRows = 16;        // fc1 / fc2 rows per workgroup (F / kXcdWgs)
// wave roles (all eight compute GRU1, one unit per thread; waves map to SIMD w mod 4):
//   0, 5..7  GRU2, one wave per SIMD: wave 0 is group g = 0, wave w ≥ 5 group g = w − 4; engine e
//            of group g owns units 4g + e (r, z in its lanes 0, 1; n, h' in lane 0) and 4g + 2 + e
//            (lanes 2, 3; lane 2), six W_ih2 gate rows in VGPRs, and publishes y, later h2 (lanes
//            0, 2 of engine 0, engine 1's values by a permlane32 swap).  Wave 0 also samples
//            (polls F2) and has W_hh1 rows 0..9; 5..7: W_hh1 rows (5, 7), the h2 gather (6), the
//            ring (7), one W_hh2 pass in VGPRs + W_hh2 LDS passes (5, 6)
//   1, 2     fc1 rows 8h..8h+7 (h = w − 1) from the polled y — polling from barrier B2 on, no
//            store of their own ahead of the poll; three W_hh2 passes in VGPRs + two from LDS
//   3, 4     fc2 rows 8h..8h+7 (h = w − 3) from the polled f1 + their fc3 partials; W_hh1 rows
//            (after wave 0's y store: not issued into GRU2 on the SIMDs shared with waves 7, 0);
//            three W_hh2 passes in VGPRs (wave 3: + two from LDS); wave 4 gathers a quarter of the
//            next step's GRU1 terms
// W_hh2 pass P = rows 2P + e (e = engine).  VGPR passes: wave w = 1..4 holds 3(w − 1)..+2, wave
// w = 5..7 holds 7 + w; LDS passes 15..23: waves 1, 2 two each (15.., 17..), wave 5 pass 19,
// wave 6 passes 20, 21, wave 3 passes 22, 23 (wave 7, which also fills the ring, reached the
// step-end barrier after the sampler with them).
constexpr int kXWaveFc1 = 1, kXWaveFc2 = 3;
constexpr int kXH2RegRows = 30;     // W_hh2 rows 0..29 in VGPRs, 30..47 in LDS
constexpr int kXH2LdsRows = 18;
static_assert(kXH2RegRows == 2 * (4 * 3 + 3 * 1), "W_hh2 VGPR passes: 3 on each fc wave, 1 on waves 5..7");
static_assert(kXH2RegRows + kXH2LdsRows == 48, "every W_hh2 row of the workgroup has one holder");
constexpr int kXRing = 4;           // steps of conditioning terms / sampler noise in LDS
constexpr int kXNoise = 16;         // 11 MoL sampler terms, padded

// Conditioning terms of one step for one workgroup (columns of the terms GEMM), floats:
//   [0,48) P1 = W_ih1·cI, [48,96) P2 = W_ih2·[cI; a2]   (index u·3 + gate, u = local unit)
//   [96,112) cI of the own units, [112,128) V1 = W1[:, R:]·a3 + b1, [128,144) V2 = W2[:, F:]·a4 + b2
//   [144,160) one-shot launches: the row-step's 11 sampler terms, padded (launch_xcd_draws writes them over
//   the GEMM's zeros, the same 16 floats in every workgroup's record); otherwise unused
enum XTerm { XT_P1 = 0, XT_P2 = 48, XT_CI = 96, XT_V1 = 112, XT_V2 = 128, XT_NZ = 144, kXTerms = 160 };
static_assert(XT_NZ + kXNoise == kXTerms, "the sampler record fills the terms record's padding");

// Hand-off vectors of one XCD (granules {tag = step + 1, value}, plain stores that stay in the
// XCD's L2, sc1 polls).  S (the GRU1 terms) is double-buffered by step parity.
enum XHop { XH_Y = 0, XH_F1 = 1, XH_F2 = 2, XH_H2 = 3, XH_S0 = 4, XH_S1 = 5, kXHops = 6 };
constexpr int kXF2Line = 32;        // granules per workgroup in the partial-logit vector
constexpr long long kXHopStride = 4096;            // granules per hop region (≥ 4·512, 32·32)
constexpr long long kXXcdStride = kXHops * kXHopStride + 512;   // granules per XCD

// Per-workgroup weight slab (floats), all rows natural (512 contiguous):
struct XcdSlab {
    int wih2;    // [8 pairs][6 rows (2q + i)][512]   W_ih2[:, :R] gate q of unit 2p + i (GRU2 group g: pairs 2g, 2g + 1)
    int w1;      // [16][512]                           fc1 rows 16c + r (y part)
    int w2;      // [16][512]                           fc2 rows 16c + r (f1 part)
    int whh2;    // [48][512]   W_hh2 rows u·3 + q (rows < kXH2RegRows in VGPRs, the rest LDS)
    int whh1;    // [48][512]                           W_hh1 rows u·3 + q (LDS-resident)
    int w3;      // [16][32]                            W3[j][16c + r] (j ≥ 30: 0)
    int q1a;     // [3][512]                            W_ih1·W_I[:, 0], gate-major (all units)
    int cst;     // [kXCst] small vectors, copied to LDS (XCst offsets)
    int total;
};

// Small per-workgroup vectors (LDS-resident), offsets within the cst block
enum XCst { XC_Q2 = 0, XC_BIH1 = 48, XC_BHH1 = 96, XC_BIH2 = 144, XC_BHH2 = 192, XC_WI0 = 240, XC_B3 = 256, kXCst = 288 };
//   q2 = W_ih2[:, :R]·W_I[:, 0] (own units), biases of both GRUs (own units, u·3 + q), W_I[:, 0]
//   of the own units, b3 (padded to 32)

// Per-workgroup state carried between time chunks (floats):
// [h1 512 | sg 2048 (terms of the next step) | gh2 48 | h2own 16 (by local unit) | x | pad]
constexpr int kXStateW = 512 + 2048 + 48 + 16 + 16;

struct XcdArgs {
    const float *slab;            // [kXcdWgs][slab.total]
    const float *terms;           // [Lc + 1][nb][kXcdWgs·kXTerms], row (t - t0)·nb + k
    const float *noise;           // [L][Bt][11] (windowed: [nz_hor][Bt][11]), row = step, or nullptr (Philox)
    float *out;                   // [Bt][L]; windowed: [Bt][out_ld], step t at column t − out_t0
    float *state;                 // [nb][kXcdWgs][kXStateW]
    unsigned long long *xg;       // [nb][kXXcdStride] granules
    int *members;                 // [kXcds] arrival counters (zeroed before the launch)
    int *ctl;                     // [0] abort, [1] code, [2] step, [3] hop, [4] wg
    unsigned long long seed;
    long long row0;               // global row id of XCD 0's row (Philox key: row0 + k)
    long long timeout_ticks;
    // Steps [t0, t0 + Lc) of a loop that goes on while t + 1 < L: the total length, or (windowed
    // launches) anything past t0 + Lc while the end is unknown — the terms then hold the row of step
    // t0 + Lc too
    int L, t0, Lc, Bt, b0, nb;
    XcdSlab s;
    unsigned *dbg;                // [nb·32][dbg_steps][kStamps] or nullptr
    int dbg_steps;
    // windowed launches (streaming sessions: a chunk of an utterance whose length may not be known
    // yet; the kernel's kWin instantiation, which alone reads these): injected draws exist for
    // steps < nz_hor, the output has its own leading dimension and time origin
    int windowed, nz_hor, out_ld, out_t0;
};

// Grouped launches (streaming sessions advancing independently, wrnn_stream_push_group): XCD k
// runs row k of a table of these in place of the launch-wide window — every hand-off of a row
// stays inside its XCD, so its step window, terms, draws, state, granules and output are its own.
// Pointers are the ROW's (the session's buffers already offset to its utterance).  The kernels'
// kGrp instantiation alone reads the table; a row with Lc = 0 takes no XCD.
struct XcdRow {
    const float *terms;           // the row's terms of step t0; step t at + (t − t0)·terms_ld (+ c·kXTerms)
    const float *noise;           // the row's draws of step 0; step t at + t·noise_ld, or nullptr (Philox)
    float *out;                   // the row's samples: step t at out[t − out_t0]
    float *state;                 // [kXcdWgs][state width of the kernel]
    unsigned long long *xg;       // [kXXcdStride] granules
    unsigned long long seed;
    long long row;                // global row id (Philox key)
    long long terms_ld;           // floats between consecutive steps: (utterances of the session)·N
    int noise_ld;                 // floats between consecutive steps of draws: (utterances of the session)·11
    int out_t0;
    int t0, Lc, L, nz_hor;        // as XcdArgs' (windowed), per row
};

struct XcdGroupArgs {
    XcdArgs a;                    // slab, members, ctl, timeout_ticks, s, nb = rows in the table; the rest unread
    XcdRow row[kXcds];
};

// List launches (wrnn_generate_list): XCD k is a LANE that runs a queue of pieces back to back
// without leaving the kernel — piece = steps [t0, t0 + Lc) of one utterance, exactly an XcdRow
// (terms_ld = N: a piece's terms rows are its own, contiguous).  The queue lives in device memory
// (eight rows already fill ≈ 1 KB of kernel arguments); the interpolation pass that fills a
// round's terms (terms_interp_list_kernel, frame_terms.hip) walks the same records: ft / at are the
// utterance's frame-term stores, nt the terms rows of the piece (its steps and, while the
// utterance goes on, the one after them).  The kernels' kLst instantiation alone reads the table.
struct XcdPiece {
    XcdRow r;
    const float *ft;              // [frames + nJ − 1][N]  W·(mel frame) rows of the utterance
    const float *at;              // [frames + 1][N]       W·(aux frame, ones) rows
    int frames, nt;
    int blk0, pad_;               // the piece's first block of the round's interpolation launch (kInterpSteps rows each)
};

struct XcdListArgs {
    XcdArgs a;                    // slab, members, ctl, timeout_ticks, s, nb = lanes; the rest unread
    const XcdPiece *pieces;       // device: every piece of the call, round-major, lane-major within a round
    int first[kXcds + 1];         // this launch: XCD k walks pieces first[k] .. first[k + 1] − 1 (none: no XCD)
};

struct XcdLds {
    int whh1, whh2, h1, h2, sg, w3, f2x, ring, nz, gh2, cst, xs, misc, total;
};

__host__ __device__ constexpr XcdLds xcd_lds_layout() {
    XcdLds l{};
    int o = 0;
    // the small per-step arrays first (offsets < 64 KiB: lane address + instruction immediate)
    l.h1 = o;    o += 512;
    l.h2 = o;    o += 512;
    l.sg = o;    o += 4 * 512;                // GRU1 terms of all units for the coming step
    l.w3 = o;    o += kXFcRows * 32;          // fc3 columns of the own f2 rows (waves 3, 4)
    l.f2x = o;   o += 64;                     // wave 4's fc3 partials, handed to wave 3: (value, tag) pairs
    l.ring = o;  o += kXRing * kXTerms;
    l.nz = o;    o += kXRing * kXNoise;
    l.gh2 = o;   o += 48;                     // W_hh2·h2 of the own units for the next step
    l.cst = o;   o += kXCst;
    l.xs = o;    o += 4;                      // x, by step parity
    l.misc = o;  o += 8;                      // [0] abort flag, [1] member index, step flags (step + 1):
                                              // [2] h2 gathered, [3] y store issued (wave 0), [4] y gathered, [5] f1 gathered
    l.whh1 = o;  o += 48 * 512;
    l.whh2 = o;  o += kXH2LdsRows * 512;
    l.total = o;
    return l;
}
static_assert(xcd_lds_layout().total * 4 <= 160 * 1024, "the XCD kernel's LDS image fits a CU's 160 KB");

// host launchers (fatchord_xcd.hip)
hipError_t launch_xcd(const XcdArgs &a, hipStream_t st);
// The sampler terms of a one-shot launch's rows [0, nb) for the n terms rows of steps [t0, t0 + n), into
// slot XT_NZ of every workgroup's record of `terms` (row dt·nb + k): the 11 terms the sampler adds to the
// logits (mol_noise_term of the Philox draw keyed (seed, row0 + k, t0 + dt, kk), or of
// noise[((t0 + dt)·Bt + b0 + k)·11 + kk] when draws are injected), zero-padded — formed once per row-step
// instead of in the step loop of every workgroup.  After the terms GEMM / interpolation of the chunk.
hipError_t launch_xcd_draws(float *terms, const float *noise, unsigned long long seed, long long row0, int nb, int Bt,
                            int b0, int t0, int n, hipStream_t st);
hipError_t launch_xcd_group(const XcdGroupArgs &g, hipStream_t st);
hipError_t launch_xcd_list(const XcdListArgs &g, hipStream_t st);
hipError_t prepare_xcd_kernel(int max_lds_bytes);
hipError_t xcd_occupancy(int *blocks_per_cu);

}  // namespace wrnn
