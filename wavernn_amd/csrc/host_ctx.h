// host_ctx.h — what the host files of the C-ABI (capi*.cpp) share: the handle, the grow-only
// buffers and staged tables it owns, the error path, the frame-rate terms pass and the few helpers
// that cross files (namespace wrnn::host; everything else is static in its file).
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/wavernn_amd.h"
#include "condition.h"
#include "deepmind_rows.h"
#include "deepmind_xcd.h"
#include "fatchord_loop.h"
#include "fatchord_rows.h"
#include "fatchord_split.h"
#include "fatchord_xcd.h"
#include "fatchord_xcdm.h"
#include "fatchord_xcds.h"
#include "frame_terms.h"

namespace wrnn {
namespace host {

// grow-only device buffer
template <typename T>
hipError_t ensure(T *&p, size_t &cap, size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) {
        hipError_t e = hipFree(p);
        if (e != hipSuccess) return e;
    }
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
}

// A device table a call fills from the host: the table, its pinned staging copy and the event that
// marks the end of the last upload (the staging copy is rewritten only after it).  reserve(n)
// returns once that upload has read the staging copy, with room for n records in both (the pinned
// copy grows by doubling); the caller then writes h[0 .. n) and upload()s.
template <typename Rec>
struct StagedTable {
    Rec *d = nullptr, *h = nullptr;
    size_t d_cap = 0, h_cap = 0;   // records
    hipEvent_t ev = nullptr;

    hipError_t reserve(size_t n) {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventSynchronize(ev);
        if (e == hipSuccess) e = ensure(d, d_cap, n);
        if (e != hipSuccess || n <= h_cap) return e;
        if (h && (e = hipHostFree(h)) != hipSuccess) return e;
        h = nullptr;
        h_cap = 0;
        e = hipHostMalloc((void **)&h, 2 * n * sizeof(Rec), hipHostMallocDefault);
        if (e == hipSuccess) h_cap = 2 * n;
        return e;
    }
    hipError_t upload(size_t n, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(d, h, n * sizeof(Rec), hipMemcpyHostToDevice, st);
        return e == hipSuccess ? hipEventRecord(ev, st) : e;
    }
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        if (ev) (void)hipEventDestroy(ev);
        d = h = nullptr;
        d_cap = h_cap = 0;
        ev = nullptr;
    }
};

}  // namespace host
}  // namespace wrnn

// One partition of the loop weights over the multi-row kernel's workgroups (see wrnn_ctx).
struct RowsPart {
    wrnn::RowsSlab rs{};
    int rU = 0, rG = 0, rUF = 0, rUC = 0, NT = 0;
    bool ok = false;
    float *d_slab = nullptr, *d_Wt = nullptr;
};

// The deepmind partition (units per workgroup, grid) and its packed slab (see wrnn_ctx::dm2)
struct DmPart {
    wrnn::DmSlab ds{};
    int dmU = 0, dmUO = 0, dmUO2 = 0, G = 0;
    bool ok = false;
    float *d_slab = nullptr;
};

struct wrnn_ctx {
    wrnn_config cfg{};
    int device = 0;
    int num_cus = 0;
    int max_lds = 0;
    int G = 0, U = 0, UF = 0, UC = 0, NMAX = 0, NK = 0, CD = 0;
    int max_rows = 0;
    wrnn::SlabLayout s{};
    std::map<std::string, std::vector<float>> w;   // loop tensors, host copies
    bool ready = false;
    unsigned long long loads = 0;                   // wrnn_set_weights calls that took a tensor (sessions bind one)
    float *d_slab = nullptr, *d_IW = nullptr, *d_Ib = nullptr;
    float *d_cI = nullptr;
    size_t cI_cap = 0;                              // floats
    unsigned long long *d_xg = nullptr;
    size_t xg_cap = 0;                              // granules
    int *d_ctl = nullptr;
    long long timeout_ticks = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    std::string err;
    // multi-row (fold-batched) path: fatchord_rows.hip
    wrnn::RowsSlab rs{};
    int rU = 0, rG = 0, rUF = 0, rUC = 0;           // rows-kernel partition (U = 4 when sparse)
    bool sparse = false;                            // GRU weights stored as nonzero 4x4 blocks
    int NT = 0, KX = 0, KA = 0;
    int KXc = 0;                                    // XCD kernels' terms-GEMM depth: [cond record | 1 0 0 0]
    bool rows_ok = false;                           // weights fit LDS with at least one row (or stream)
    bool rows_gw = false;                           // dense weights exceed LDS: the slab is streamed from HBM
    float *d_rslab = nullptr, *d_Wt = nullptr;      // per-workgroup slabs, terms-GEMM weights [G·NT][KX]
    float *d_X = nullptr, *d_T = nullptr, *d_act = nullptr, *d_state = nullptr;
    size_t X_cap = 0, T_cap = 0, act_cap = 0, state_cap = 0;   // floats
    unsigned *d_flags = nullptr;                    // [2 row groups][kRowsHops][kFlagSlots][kFlagStride]
    unsigned long long *d_xr = nullptr;             // x granules, [2 row groups][kXReps][kXRepStride]
    unsigned long long *d_gact = nullptr;           // rows granule mode: [2 row groups][kRowsHops][gstride]
    size_t gact_cap = 0;
    // the same weights over G/2 workgroups (twice the units each) for two row groups per launch
    // (large B: halves the activation rows every workgroup streams per stage); swapped into the
    // r* fields above while in use
    RowsPart g2{};
    rocblas_handle blas = nullptr;
    int last_path = 0;                              // 1 = latency, 2 = rows, 3 = deepmind, 4 = split, 5 = xcd, 6 = xcd sparse
    // what the last multi-row call (generate_rows, generate_dm, a rows session's push) chose: row groups,
    // row blocks, rows and tile rows of its first block; zeros after any other call (set_last_path)
    int last_row_groups = 0, last_row_blocks = 0, last_block_rows = 0, last_tile_rows = 0;
    // deepmind_version (WRNN_MODE_DM): deepmind_rows.hip
    wrnn::DmSlab ds{};
    int dmU = 0, dmUO = 0, dmUO2 = 0;
    bool dm = false;
    bool dm_gw = false;                             // the DM slab exceeds LDS: streamed from HBM
    float *d_dmslab = nullptr;
    DmPart dm2{};                                   // G/2 workgroups, twice the units: two row groups per launch
    unsigned *d_dmflags = nullptr;
    unsigned long long *d_dmxg = nullptr;
    size_t dmflags_cap = 0, dmxg_cap = 0;
    // batch-1 MoL role-split kernel: fatchord_split.hip
    bool split_ok = false;
    int sGg = 0, sGf = 0;
    wrnn::SplitGruSlab sgs{};
    wrnn::SplitFcSlab sfs{};
    float *d_sgslab = nullptr, *d_sfslab = nullptr, *d_sWt = nullptr;
    // XCD-resident MoL kernel (rnn / fc 512): fatchord_xcd.hip
    bool xcd_ok = false;
    wrnn::XcdSlab xs{};
    float *d_xslab = nullptr, *d_xWt = nullptr, *d_xstate = nullptr;
    size_t xstate_cap = 0;
    unsigned long long *d_xgx = nullptr;
    int *d_members = nullptr;
    // XCD-resident MoL kernel for rnn 896 with 4x4 block-sparse GRU weights: fatchord_xcds.hip
    // (shares the d_x* buffers: the dense one needs rnn 512); cap = dims and device fit, ok =
    // the loaded weights are block-sparse with <= kSNB nonzero blocks per gate block-row
    bool xcds_cap = false, xcds_ok = false;
    wrnn::XcdsSlab xss{};
    // XCD-resident many-row MoL kernel (rnn / fc 512, MFMA): fatchord_xcdm.hip; shares the XCD
    // kernel's terms-GEMM weights (d_xWt)
    bool xcdm_ok = false;
    int xcdm_nq = 0;                                // largest co-resident quad count (rows per XCD / 4)
    wrnn::XcdmSlab xms{};
    float *d_xmslab = nullptr, *d_xmstate = nullptr, *d_xmnoise = nullptr;
    float *d_xmWt = nullptr;   // many-row kernel's terms-GEMM weights: the first kMRing rows of each workgroup's record
    size_t xmnoise_cap = 0;
    // XCD-resident deepmind kernel (hidden 896, quantisation 256, MFMA): deepmind_xcd.hip
    bool dx_ok = false;
    float *d_dxslab = nullptr, *d_dxstate = nullptr, *d_dxnoise = nullptr;
    size_t dxnoise_cap = 0;
    unsigned long long *d_dxxg = nullptr;
    unsigned long long *d_xmxg = nullptr;
    // frame-rate conditioning terms (wrnn_generate_frames, frame_terms.hip): the cascade's
    // per-phase frame weights, W·(mel frame) and W·(aux frame, ones) rows, their GEMM input
    // records, and the per-sample conditioning of the paths that still take it
    float *d_coef = nullptr, *d_FT = nullptr, *d_AT = nullptr, *d_frec = nullptr, *d_cond = nullptr;
    size_t coef_cap = 0, FT_cap = 0, AT_cap = 0, frec_cap = 0, cond_cap = 0;
    std::vector<float> coef_host;                   // the table d_coef holds (re-uploaded when it changes)
    // list calls (wrnn_generate_list*): per-utterance frame-term stores (one arena), recurrent-state
    // records and granule regions, and the lane list's piece table
    float *d_larena = nullptr, *d_lstate = nullptr;
    size_t larena_cap = 0, lstate_cap = 0;
    unsigned long long *d_lxg = nullptr;
    size_t lxg_cap = 0;
    wrnn::host::StagedTable<wrnn::XcdPiece> ltab;
    // wide streaming groups (wrnn_stream_open_wide), wide and folded lists: the many-row kernel's
    // grouped instantiation (of the handle's head, MoL or RAW) is co-resident; the row tables of
    // one call's launches
    bool xcdmg_ok = false;
    wrnn::host::StagedTable<wrnn::XcdmRow> wtab;
};

namespace wrnn {
namespace host {

constexpr int kCtlWords = 8;

inline int fail(wrnn_t *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}

// The kernel a call runs (wrnn_info.last_path); the multi-row runners fill the last_row_* fields after it
inline void set_last_path(wrnn_t *h, int path) {
    h->last_path = path;
    h->last_row_groups = h->last_row_blocks = h->last_block_rows = h->last_tile_rows = 0;
}
// One row block of a multi-row call: the first one's choices are what wrnn_info reports
inline void note_row_block(wrnn_t *h, int groups, int rows, int tile) {
    if (h->last_row_blocks++ == 0) {
        h->last_row_groups = groups;
        h->last_block_rows = rows;
        h->last_tile_rows = tile;
    }
}

#define HIP_TRY(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail((h), WRNN_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

inline int grow(wrnn_t *h, float *&p, size_t &cap, size_t n) {
    HIP_TRY(h, ensure(p, cap, n));
    return WRNN_OK;
}

// ---- capi.cpp: what the runners need of the layouts and partitions
size_t lds_bytes_for(const wrnn_ctx &h, int Bc);
size_t rows_lds_bytes(const wrnn_ctx &h, int B, int TB, bool head_lds = true);
int rows_tile_for(const wrnn_ctx &h, int B, bool head_lds = true);
bool rows_terms_composed(const wrnn_ctx &h);
int rows_terms_kx(const wrnn_ctx &h);
size_t dm_lds_bytes(const wrnn_ctx &h, int B, int TB);
int dm_tile_for(const wrnn_ctx &h, int B);
size_t split_lds_bytes(const wrnn_ctx &h);
// (record rows, first input column, depth) of the many-row kernel's three segmented terms GEMMs
struct XcdmGemm {
    int row0, rows, col0, k;
};
void xcdm_terms_gemms(const wrnn_ctx &h, XcdmGemm (&g)[3]);

// Swaps a partition in for a scope
void swap_part(wrnn_ctx &h, RowsPart &p);
struct PartScope {
    wrnn_ctx &h;
    RowsPart &p;
    bool on;
    PartScope(wrnn_ctx &h_, RowsPart &p_, bool on_) : h(h_), p(p_), on(on_) {
        if (on) swap_part(h, p);
    }
    ~PartScope() {
        if (on) swap_part(h, p);
    }
};
void swap_dm(wrnn_ctx &h, DmPart &p);
struct DmScope {
    wrnn_ctx &h;
    DmPart &p;
    bool on;
    DmScope(wrnn_ctx &h_, DmPart &p_, bool on_) : h(h_), p(p_), on(on_) {
        if (on) swap_dm(h, p);
    }
    ~DmScope() {
        if (on) swap_dm(h, p);
    }
};

// ---- capi_loops.cpp
// The WRNN_TERMS_MB budget (default 8192 MiB) in floats; every launch loop divides it by its own
// floats per step (tools/list_throughput.py restates those formulas).
double terms_budget_floats();
// rocBLAS on the call's stream (the handle is created at first use)
int blas_on(wrnn_t *h, hipStream_t st);
// The frame weights on the device: uploaded when they differ from the table d_coef holds
int upload_coef(wrnn_t *h, const std::vector<float> &coef, hipStream_t st);
// The loop path for B rows (WRNN_PATH=xcd|xcdm|split|latency|rows forces one: tests, benchmarks).
enum LoopPath { P_LATENCY = 1, P_ROWS = 2, P_DM = 3, P_SPLIT = 4, P_XCD = 5, P_XCDS = 6, P_XCDM = 7, P_DX = 8 };
LoopPath choose_path(const wrnn_t *h, int B);
// The multi-row kernel's launch loop in pieces, shared by generate_rows and the rows sessions
// (capi_stream.cpp).  The caller holds the PartScope of rows_grouped(h, B) around all of them.
// RowsBlock: what generate_rows decides per row block — the one- or two-group partition by row count,
// tile size and head_lds, granule or bulk hops, the steps per launch under WRNN_TERMS_MB.
struct RowsBlock {
    int ng, Bl, Bg, Bg1;          // row groups; rows of the block, of group 0 and of group 1
    int N, KXg, TB, SW, Lc_max;
    bool mol, head_lds, gran, f2g;
    long long gstride;
    size_t T_grp, act_grp, state_grp;   // floats per group of the terms, the bulk activations, the carried state
};
// What a launch reads and writes: cond [..][Bt][CD] whose first record is step cond_t0, rows
// [b0, b0 + Bl) of it; noise [steps][Bt][NK] by absolute step or nullptr (Philox); sample of row b and
// step t at out[(b0 + b)·out_ld + t] (labels likewise, or nullptr); state [ng][state_grp] carried
// from launch to launch (read when t0 > 0)
struct RowsRun {
    const float *cond, *noise;
    float *out, *state;
    int32_t *labels;
    int cond_t0, Bt, b0, out_ld;
    uint64_t seed;
    int64_t row_offset;
    unsigned *dbg;
    int dbg_steps;
};
bool rows_grouped(const wrnn_ctx &h, int B);
int rows_hop_areas(wrnn_t *h);
int rows_block(wrnn_t *h, bool grouped, int rows_left, int steps, RowsBlock *out);
int rows_reset(wrnn_t *h, const RowsBlock &k, bool act, hipStream_t st);
int rows_chunk(wrnn_t *h, const RowsBlock &k, const RowsRun &r, int t0, int Lc, hipStream_t st);
// The upsample config of a call against the handle's feat / aux dims, and its 1..4 scales with a
// scale and taps each (h may be null there: no message is kept)
int check_upsample_dims(wrnn_t *h, const wrnn_upsample_cfg *ucfg);
int check_upsample_scales(wrnn_t *h, const wrnn_upsample_cfg *ucfg);
bool frame_weights(const wrnn_upsample_cfg &c, int *hop_out, int *nJ_out, int *jlo_out, std::vector<float> &coef);
// frame_weights, or the refusal of a cascade without an exact frame-rate form
int frame_form(wrnn_t *h, const wrnn_upsample_cfg *ucfg, int *hop, int *nJ, int *jlo, std::vector<float> &coef);

// ---- capi_stream.cpp: what the wide and folded lists share with the wide groups
// Why a MoL or RAW handle has no grouped many-row form, or "" when it has one
std::string wide_refusal(const wrnn_t *h);
// One persistent launch of a wide push or list: first step, steps, rows
struct WideLaunch {
    int off, Lc, rows;
};
// the launches of at most Lc_max steps that cover steps [prev, c) with `rows` rows, appended
void push_launches(std::vector<WideLaunch> &ls, long long prev, long long c, int Lc_max, int rows);
// (first, steps, rows) of the launches into the caller's arrays (each may be null), `cap` at most → their count
int emit_launches(const std::vector<WideLaunch> &ls, int *first, int *steps, int *rows, int cap);
size_t fold_tab_records(size_t ntab);
int wide_tab_reserve(wrnn_t *h, size_t ntab);
int wide_run_launches(wrnn_t *h, const std::vector<WideLaunch> &ls, size_t ntab, const float *d_coef, int hop, int nJ,
                      bool raw, int K, hipStream_t st, bool folds = false);

// ---- frame-rate conditioning terms (frame_terms.hip) -------------------------------------
// A loop row's terms come from its utterance's frame rows: row r is utterance r / nf starting at
// step (r % nf)·stride (fold_with_overlap, fatchord_version.py:317-330; unbatched nf = 1).
struct FrameSrc {
    const float *mel = nullptr, *aux = nullptr;   // [U][feat][NF], [U][4·aux][NF] (device)
    int U = 0, NF = 0, nf = 1, stride = 0;
    int rb = 0;                                   // launch row j is row rb + j of the U·nf (wrnn_generate_frames_rows)
    int hop = 1, nJ = 1, jlo = 0;
    const float *coef = nullptr;                  // [hop][nJ] (device)
};

// FT [NF + nJ − 1][U][N] = W·[mel frame | 0 | 0] and AT [NF + 1][U][N] = W·[0 | aux frame | 1]
// (row NF: W·[0 | 0 | 1]) through the path's own terms GEMM(s): gemm(X, m, C) writes
// C[m][N] = W·X for X [m][KX] as pack_cond_input lays it out (`split`).
// FT_dst / AT_dst: stores of the caller's in place of the handle's d_FT / d_AT (the list calls:
// one pair per utterance in their arena); the launches and their shapes are the same.
template <typename Gemm>
int frame_terms(wrnn_t *h, const FrameSrc &fs, int N, int KX, int split, hipStream_t st, Gemm gemm,
                float *FT_dst = nullptr, float *AT_dst = nullptr) {
    const int feat = h->cfg.feat_dims, A4 = h->CD - feat;
    const int NFF = fs.NF + fs.nJ - 1, NFA = fs.NF + 1, fmax = std::max(NFF, NFA);
    if (grow(h, h->d_frec, h->frec_cap, (size_t)fmax * fs.U * h->CD) ||
        grow(h, h->d_X, h->X_cap, (size_t)fmax * fs.U * KX))
        return WRNN_EHIP;
    if (!FT_dst) {
        if (grow(h, h->d_FT, h->FT_cap, (size_t)NFF * fs.U * N) || grow(h, h->d_AT, h->AT_cap, (size_t)NFA * fs.U * N))
            return WRNN_EHIP;
        FT_dst = h->d_FT;
        AT_dst = h->d_AT;
    }
    for (int kind = 0; kind < 2; ++kind) {
        const int frames = kind ? NFA : NFF;
        HIP_TRY(h, launch_frame_cond(fs.mel, fs.aux, fs.U, feat, A4, fs.NF, frames, fs.jlo, kind, h->d_frec, st));
        HIP_TRY(h, launch_pack_cond_input(h->d_frec, h->CD, fs.U, 0, fs.U, 0, frames, KX, h->d_X, st, split,
                                          kind ? 1.0f : 0.0f));
        if (int rc = gemm(h->d_X, frames * fs.U, kind ? AT_dst : FT_dst)) return rc;
    }
    return WRNN_OK;
}

}  // namespace host
}  // namespace wrnn
