// capi_loops.cpp — the one-shot loop runners of the C-ABI host: one generate_* per kernel, the choice
// of the path, wrnn_generate and the frame-rate entry points (wrnn_frame_weights, wrnn_generate_frames*).
#include "host_ctx.h"

using namespace wrnn;
using namespace wrnn::host;

namespace {

// WRNN_DEBUG_STAMPS buffer: freed on every exit path (an early HIP_TRY / fail() return included);
// the dump helpers take ownership by resetting p first
struct DbgBuf {
    unsigned *p = nullptr;
    DbgBuf() = default;
    DbgBuf(const DbgBuf &) = delete;
    DbgBuf &operator=(const DbgBuf &) = delete;
    ~DbgBuf() {
        if (p) (void)hipFree(p);
    }
    unsigned *release() {
        unsigned *q = p;
        p = nullptr;
        return q;
    }
};

// WRNN_DEBUG_FILE (default wrnn_stamps.bin): the int32 header — {G, steps, kStamps} of the per-workgroup
// stamps, {waves, steps, stamps} of the per-wave ones (many-row / deepmind kernels) — then the n stamps
int dump_stamps(wrnn_t *h, DbgBuf &dbg, size_t n, const int (&hdr)[3], hipStream_t st) {
    std::vector<unsigned> host(n);
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, hipMemcpy(host.data(), dbg.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipFree(dbg.release()));
    const char *path = std::getenv("WRNN_DEBUG_FILE");
    if (FILE *f = std::fopen(path ? path : "wrnn_stamps.bin", "wb")) {
        std::fwrite(hdr, sizeof(hdr), 1, f);
        std::fwrite(host.data(), 4, host.size(), f);
        std::fclose(f);
    }
    return WRNN_OK;
}

// B rows through the multi-row kernel: row blocks of <= kRowsMax rows per launch, time chunks
// sized so the precomputed terms stay within WRNN_TERMS_MB (default 8192 MiB).  Blocks of
// >= kGroupRows rows run as two row groups of half the rows on G/2 workgroups each (the grouped
// partition, dense weights only; WRNN_ROW_GROUPS=1|2 forces one or the other).  Measured on
// MI355X (MoL 512, us/step, one group → two): B=2 17.2 → 15.7, B=10 18.3 → 16.9, B=32 26.6 →
// 19.5, B=115 51.2 → 40.2: half the rows streamed per stage and half the flags per hop.
// The per-block choices, the hop-area reset and the per-time-chunk body are wrnn::host::rows_block,
// rows_reset and rows_chunk below: a rows session (capi_stream.cpp) runs its steps through the same.
constexpr int kGroupRows = 2;
constexpr size_t kRowsGranMax = 4096;   // values per row group and hop up to which hops use granules
constexpr size_t kDmGranMax = 8192;     // the same for the deepmind kernel (one poll round of all waves)

int generate_rows(wrnn_t *h, const float *cond, int B, int L, const float *noise, uint64_t seed, int64_t row_offset,
                  float *out, int32_t *labels, hipStream_t st) {
    const bool grouped = rows_grouped(*h, B);
    PartScope ps(*h, h->g2, grouped);          // h->r*, rs, NT, d_rslab, d_Wt = the grouped partition
    if (int rc = rows_hop_areas(h)) return rc;
    if (int rc = blas_on(h, st)) return rc;
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = dbg_env ? std::min(L, std::atoi(dbg_env)) : 0;
    DbgBuf dbg;
    if (dbg_steps > 0) {
        HIP_TRY(h, hipMalloc(&dbg.p, (size_t)h->rG * dbg_steps * kStamps * 4));
        HIP_TRY(h, hipMemsetAsync(dbg.p, 0, (size_t)h->rG * dbg_steps * kStamps * 4, st));
    }
    for (int b0 = 0; b0 < B;) {
        RowsBlock k;
        if (int rc = rows_block(h, grouped, B - b0, L, &k)) return rc;
        note_row_block(h, k.ng, k.Bl, k.TB);
        if (grow(h, h->d_X, h->X_cap, (size_t)k.Lc_max * k.Bg * k.KXg) || grow(h, h->d_T, h->T_cap, k.ng * k.T_grp) ||
            grow(h, h->d_act, h->act_cap, k.ng * k.act_grp) || grow(h, h->d_state, h->state_cap, k.ng * k.state_grp))
            return WRNN_EHIP;
        if (int rc = rows_reset(h, k, false, st)) return rc;
        RowsRun r{};
        r.cond = cond;
        r.cond_t0 = 0;
        r.Bt = B;
        r.b0 = b0;
        r.noise = noise;
        r.out = out;
        r.out_ld = L;
        r.labels = labels;
        r.state = h->d_state;
        r.seed = seed;
        r.row_offset = row_offset;
        for (int t0 = 0; t0 < L; t0 += k.Lc_max) {
            const int Lc = std::min(k.Lc_max, L - t0);
            r.dbg = (b0 == 0 && t0 == 0) ? dbg.p : nullptr;
            r.dbg_steps = std::min(dbg_steps, Lc);
            if (int rc = rows_chunk(h, k, r, t0, Lc, st)) return rc;
        }
        b0 += k.Bl;
    }
    if (dbg.p) return dump_stamps(h, dbg, (size_t)h->rG * dbg_steps * kStamps, {h->rG, dbg_steps, kStamps}, st);
    return WRNN_OK;
}

// deepmind_version: B rows (utterances) in row groups of <= kRowsMax, one launch each
// deepmind rows through the XCD-resident kernel: up to kDxRowsMax rows per launch (launch row r
// on XCD r % 8); Philox draws precomputed per time chunk (≤ WRNN_DM_NOISE_MB, default 2 GiB: config
// 5's 32 rows × 16 000 steps are 1 GiB of draws, one fill and ONE persistent launch — with 64 MiB
// chunks the call was 16 launches, ≈ 0.24 µs per step of relaunch, prologue and fill; the draws of
// a step are read once per XCD, ≈ 10 GB/s from HBM, so they need not stay in the Infinity Cache);
// the recurrent state carried per workgroup in d_dxstate.
int generate_dx(wrnn_t *h, int B, int L, const float *noise, uint64_t seed, int64_t row_offset, float *out,
                int32_t *labels, hipStream_t st) {
    const size_t xg_words = (size_t)kXcds * kDxXcdStride;
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    if (!h->d_dxxg) HIP_TRY(h, hipMalloc(&h->d_dxxg, xg_words * 8));
    if (!h->d_dxstate) HIP_TRY(h, hipMalloc(&h->d_dxstate, (size_t)kXcds * kXcdWgs * kDxStateW * sizeof(float)));
    const char *mb_env = std::getenv("WRNN_DM_NOISE_MB");
    const double budget = (mb_env ? std::atof(mb_env) : 2048.0) * (1 << 20) / 4.0;   // floats
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = (dbg_env && std::atoi(dbg_env) > 0 && L >= kDxDbgSkip + kDxDbgSteps) ? kDxDbgSteps : 0;
    const size_t dbg_n = (size_t)kXcds * kXcdWgs * kDxWaves * dbg_steps * kDxStamps;
    DbgBuf dbg;
    if (dbg_steps > 0) {
        HIP_TRY(h, hipMalloc(&dbg.p, dbg_n * 4));
        HIP_TRY(h, hipMemsetAsync(dbg.p, 0, dbg_n * 4, st));
    }
    for (int b0 = 0; b0 < B; b0 += kDxRowsMax) {
        const int nb = std::min(kDxRowsMax, B - b0);
        const int Lc_max = noise ? L : (int)std::max(1.0, std::min((double)L, budget / ((double)nb * 2 * kDxQ)));
        if (!noise && grow(h, h->d_dxnoise, h->dxnoise_cap, (size_t)Lc_max * nb * 2 * kDxQ)) return WRNN_EHIP;
        HIP_TRY(h, hipMemsetAsync(h->d_dxxg, 0, xg_words * 8, st));   // tags restart at 1
        for (int t0 = 0; t0 < L; t0 += Lc_max) {
            const int Lc = std::min(Lc_max, L - t0);
            HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
            DxArgs a{};
            a.slab = h->d_dxslab;
            if (noise) {   // injected [L][B][2Q]
                a.noise = noise;
                a.nz_t0 = 0;
                a.nz_ts = B;
                a.nz_b0 = b0;
            } else {       // Philox Exp(1) draws of this chunk ([Lc][nb][2Q]), keyed as every kernel keys them
                HIP_TRY(h, launch_philox_fill(h->d_dxnoise, seed, row_offset + b0, nb, t0, Lc, 2 * kDxQ, 0, st));
                a.noise = h->d_dxnoise;
                a.nz_t0 = t0;
                a.nz_ts = nb;
                a.nz_b0 = 0;
            }
            a.out = out;
            a.labels = labels;
            a.state = h->d_dxstate;
            a.xg = h->d_dxxg;
            a.members = h->d_members;
            a.ctl = h->d_ctl;
            a.timeout_ticks = h->timeout_ticks;
            a.L = L;
            a.t0 = t0;
            a.Lc = Lc;
            a.Bt = B;
            a.b0 = b0;
            a.nb = nb;
            a.s = dx_slab_layout();
            a.dbg = (b0 == 0 && t0 == 0 && Lc >= kDxDbgSkip + kDxDbgSteps) ? dbg.p : nullptr;
            HIP_TRY(h, launch_dx(a, st));
        }
    }
    if (dbg.p) return dump_stamps(h, dbg, dbg_n, {kXcds * kXcdWgs * kDxWaves, dbg_steps, kDxStamps}, st);
    return WRNN_OK;
}

int generate_dm(wrnn_t *h, int B, int L, const float *noise, uint64_t seed, int64_t row_offset, float *out,
                int32_t *labels, hipStream_t st) {
    // two row groups per launch (G/2 workgroups each) unless WRNN_ROW_GROUPS=1 or one row
    const char *gran_env = std::getenv("WRNN_ROWS_GRANULES");
    const int gran_force = gran_env ? std::atoi(gran_env) : -1;
    const char *grp_env = std::getenv("WRNN_ROW_GROUPS");
    const bool grouped = h->dm2.ok && B >= 2 && !(grp_env && std::atoi(grp_env) == 1);
    DmScope sc(*h, h->dm2, grouped);
    const int ng = grouped ? 2 : 1;
    const int S = h->cfg.rnn_dims / 2, Q = h->cfg.n_classes;
    const size_t flag_words = (size_t)kDmHops * kFlagSlots * kFlagStride, xg_words = (size_t)2 * kXReps * kXRepStride;
    for (int b0 = 0; b0 < B;) {
        int Bl = std::min(B - b0, kRowsMax);
        auto group_rows = [&](int bl, int g) { const int b_0 = (bl + ng - 1) / ng; return g == 0 ? b_0 : bl - b_0; };
        while (Bl > 1 && dm_tile_for(*h, group_rows(Bl, 0)) == 0) --Bl;
        // two groups: never leave one row for the next block (rows_block: 257 rows are 255 + 2)
        if (ng == 2 && B - b0 - Bl == 1 && Bl > 2) --Bl;
        const int Bg = group_rows(Bl, 0);
        const int TB = dm_tile_for(*h, Bg);
        if (TB == 0) return fail(h, WRNN_EUNSUPPORTED, "DM: one row of state does not fit LDS");
        note_row_block(h, ng, Bl, TB);
        const int SW = dm_state_width(h->dmU);
        const size_t act_grp = (size_t)kDmHops * 2 * Bg * h->KA, state_grp = (size_t)h->G * Bg * SW + 2 * Bg;
        if (grow(h, h->d_act, h->act_cap, ng * act_grp) || grow(h, h->d_state, h->state_cap, ng * state_grp))
            return WRNN_EHIP;
        HIP_TRY(h, ensure(h->d_dmflags, h->dmflags_cap, 2 * flag_words));
        HIP_TRY(h, ensure(h->d_dmxg, h->dmxg_cap, 2 * xg_words));
        HIP_TRY(h, hipMemsetAsync(h->d_dmflags, 0, ng * flag_words * 4, st));
        HIP_TRY(h, hipMemsetAsync(h->d_dmxg, 0, ng * xg_words * 8, st));
        // granule hand-offs while a group's hop vector is small (kDmGranMax values);
        // WRNN_ROWS_GRANULES=0|1 forces bulk / granules
        const bool gran = gran_force == 1 || (gran_force != 0 && (size_t)Bg * h->KA <= kDmGranMax);
        const long long gstride = (((long long)Bg * h->KA + kDmGranPad + 15) / 16) * 16;
        if (gran) {
            HIP_TRY(h, ensure(h->d_gact, h->gact_cap, (size_t)ng * kDmHops * gstride));
            HIP_TRY(h, hipMemsetAsync(h->d_gact, 0, (size_t)ng * kDmHops * gstride * 8, st));
        }
        DmArgs a{};
        a.slab = h->d_dmslab;
        a.noise = noise;
        a.out = out;
        a.labels = labels;
        a.act = h->d_act;
        a.flags = h->d_dmflags;
        a.xg = h->d_dmxg;
        a.gact = gran ? h->d_gact : nullptr;
        a.gstride = gstride;
        a.state = h->d_state;
        a.ctl = h->d_ctl;
        a.seed = seed;
        a.row0 = row_offset + b0;
        a.timeout_ticks = h->timeout_ticks;
        a.L = L;
        a.t0 = 0;
        a.Lc = L;
        a.B = Bg;
        a.Bt = B;
        a.b0 = b0;
        a.H = 2 * S;
        a.S = S;
        a.Q = Q;
        a.U = h->dmU;
        a.UO = h->dmUO;
        a.UO2 = h->dmUO2;
        a.G = h->G;
        a.TB = TB;
        a.KA = h->KA;
        a.s = h->ds;
        a.gw = h->dm_gw ? 1 : 0;
        DmGroup g1{};
        if (grouped) {
            g1.act = h->d_act + act_grp;
            g1.flags = h->d_dmflags + flag_words;
            g1.xg = h->d_dmxg + xg_words;
            g1.gact = gran ? h->d_gact + (size_t)kDmHops * gstride : nullptr;
            g1.state = h->d_state + state_grp;
            g1.row0 = row_offset + b0 + Bg;
            g1.B = group_rows(Bl, 1);
            g1.b0 = b0 + Bg;
        }
        HIP_TRY(h, launch_dm(a, grouped ? &g1 : nullptr, dm_lds_bytes(*h, Bg, TB), st));
        b0 += Bl;
    }
    return WRNN_OK;
}

// One MoL row through the role-split kernel: time chunks sized so terms + GEMM input stay within
// WRNN_TERMS_MB (default 8192 MiB).  Each chunk's terms cover one step past its end (step t's
// launch publishes the GRU1 terms of t + 1); the recurrent state is carried in d_state.
int generate_split(wrnn_t *h, const float *cond, int B, int L, const float *noise, uint64_t seed,
                   int64_t row_offset, float *out, hipStream_t st) {
    const wrnn_config &c = h->cfg;
    const int R = c.rnn_dims, A = c.aux_dims, G = h->sGg + h->sGf, N = G * kSplitTerms;
    if (int rc = blas_on(h, st)) return rc;
    const double budget = terms_budget_floats();
    const int Lc_max = (int)std::max(1.0, std::min((double)L, budget / (double)(N + h->KX) - 1.0));
    const char *rep_env = std::getenv("WRNN_REPLICAS");
    // 4 replicas of every hand-off vector (profiles/r02_split_rep_sweep.log, two rounds): 5.73/5.79 us/step
    // vs 5.71/5.80 at 8, 5.75/5.90 at 2, 6.1-6.3 at 3, 6 and 16, 7.2 at 32; every count parity-green
    const int reps = std::max(1, std::min(32, rep_env ? std::atoi(rep_env) : 4));
    const long long vec_max = std::max<long long>({(long long)kTermsPerUnit * R, (long long)R, (long long)c.fc_dims,
                                                   (long long)(R / kSplitUnits) * kYLine,
                                                   (long long)h->sGf * kSplitLogitLine});
    const long long rep_stride = (((vec_max + kOverRead) * 8 + 65535) / 65536) * 65536 / 8;
    const size_t need_xg = (size_t)kSplitHops * reps * rep_stride;
    HIP_TRY(h, ensure(h->d_xg, h->xg_cap, need_xg));
    if (grow(h, h->d_X, h->X_cap, (size_t)(Lc_max + 1) * h->KX) || grow(h, h->d_T, h->T_cap, (size_t)(Lc_max + 1) * N) ||
        grow(h, h->d_state, h->state_cap, (size_t)G * split_state_w(R)))
        return WRNN_EHIP;
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = dbg_env ? std::min(L, std::atoi(dbg_env)) : 0;
    DbgBuf dbg;
    if (dbg_steps > 0) {
        HIP_TRY(h, hipMalloc(&dbg.p, (size_t)G * dbg_steps * kStamps * 4));
        HIP_TRY(h, hipMemsetAsync(dbg.p, 0, (size_t)G * dbg_steps * kStamps * 4, st));
    }
    const float one = 1.0f, zero = 0.0f;
    for (int b0 = 0; b0 < B; ++b0) {
        HIP_TRY(h, hipMemsetAsync(h->d_xg, 0, need_xg * 8, st));
        for (int t0 = 0; t0 < L; t0 += Lc_max) {
            const int Lc = std::min(Lc_max, L - t0);
            const int rows = std::min(Lc + 1, L - t0);     // terms rows: steps [t0, t0 + rows)
            HIP_TRY(h, launch_ci_gemm(cond, h->CD, B, b0, 1, t0, rows, h->d_IW, 1 + c.feat_dims + A, h->d_Ib, R,
                                      c.feat_dims + A, h->d_X, h->KX, st));
            HIP_TRY(h, launch_pack_terms_input(cond, h->CD, B, b0, 1, t0, rows, c.feat_dims, A, R, h->KX, h->d_X, st));
            if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, rows, h->KX, &one,
                              h->d_sWt, h->KX, h->d_X, h->KX, &zero, h->d_T, N) != rocblas_status_success)
                return fail(h, WRNN_EHIP, "rocblas_sgemm (conditioning terms) failed");
            SplitArgs a{};
            a.gslab = h->d_sgslab;
            a.fslab = h->d_sfslab;
            a.terms = h->d_T;
            a.noise = noise;
            a.out = out;
            a.state = h->d_state;
            a.xg = h->d_xg;
            a.ctl = h->d_ctl;
            a.seed = seed;
            a.row0 = row_offset + b0;
            a.timeout_ticks = h->timeout_ticks;
            a.rep_stride = rep_stride;
            a.L = L;
            a.t0 = t0;
            a.Lc = Lc;
            a.Bt = B;
            a.b0 = b0;
            a.Gg = h->sGg;
            a.Gf = h->sGf;
            a.reps = reps;
            a.gs = h->sgs;
            a.fs = h->sfs;
            a.dbg = (b0 == 0 && t0 == 0) ? dbg.p : nullptr;
            a.dbg_steps = std::min(dbg_steps, Lc);
            HIP_TRY(h, launch_split(a, split_lds_bytes(*h), st));
        }
    }
    if (dbg.p) return dump_stamps(h, dbg, (size_t)G * dbg_steps * kStamps, {G, dbg_steps, kStamps}, st);
    return WRNN_OK;
}

// MoL rows through the XCD-resident kernel: up to 8 rows per launch (row k on XCD k), time
// chunks sized so terms + GEMM input stay within WRNN_TERMS_MB (default 8192 MiB).  Each chunk's
// terms cover one step past its end (step t publishes the GRU1 terms of t + 1); the recurrent
// state is carried per workgroup in d_xstate.
// The one-row-per-XCD kernels (fatchord_xcd: dense rnn 512, fatchord_xcds: block-sparse rnn 896)
// share this launch loop: rows in groups of 8 (one per XCD), time chunks whose precomputed terms
// fit the WRNN_TERMS_MB budget, one terms GEMM per chunk (one step ahead: the kernels prefetch
// the terms of step t + 1), the recurrent state carried per workgroup between chunks.
// n_terms = terms per workgroup and step, state_w = carried floats per workgroup.
template <typename Args, typename Slab>
int generate_xcd_rows(wrnn_t *h, const float *cond, const FrameSrc *fs, int B, int L, const float *noise,
                      uint64_t seed, int64_t row_offset, float *out, hipStream_t st, int n_terms, int state_w,
                      const Slab &slab, hipError_t (*launch)(const Args &, hipStream_t)) {
    const int N = kXcdWgs * n_terms;
    constexpr bool kPanels = std::is_same_v<Args, XcdArgs>;   // the terms GEMM in whole panels (below)
    // 8192 row-steps (168 MB of terms): 20 000 steps of 8 rows take 3.155 µs/step with the GEMM, as with one
    // GEMM of all columns; panels of 512 or 2048 take 3.25 (rocBLAS's kernels for those shapes)
    constexpr int kTermsPanel = 8192;
    if (int rc = blas_on(h, st)) return rc;
    if (fs) {   // frame-rate terms: W·(frames) once, then per chunk the nJ-tap sum (frame_terms.hip)
        const float one = 1.0f, zero = 0.0f;
        const int rc = frame_terms(h, *fs, N, h->KXc, 0, st, [&](const float *X, int m, float *C) -> int {
            if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, m, h->KXc, &one,
                              h->d_xWt, h->KXc, X, h->KXc, &zero, C, N) != rocblas_status_success)
                return fail(h, WRNN_EHIP, "rocblas_sgemm (frame terms) failed");
            return WRNN_OK;
        });
        if (rc) return rc;
    }
    const double budget = terms_budget_floats();
    const size_t xg_words = (size_t)kXcds * kXXcdStride;
    // each buffer under its own check: generate_xcdm / generate_dx allocate d_members too
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    if (!h->d_xgx) HIP_TRY(h, hipMalloc(&h->d_xgx, xg_words * 8));
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = dbg_env ? std::min(L, std::atoi(dbg_env)) : 0;
    DbgBuf dbg;
    int dbg_G = 0;
    const float one = 1.0f, zero = 0.0f;
    for (int b0 = 0; b0 < B; b0 += kXcds) {
        const int nb = std::min(kXcds, B - b0);
        const int Lc_max = (int)std::max(1.0, std::min((double)L, budget / ((double)nb * (N + h->KXc)) - 1.0));
        // dense kernel: the terms GEMM runs in panels of kTermsPanel row-steps, the last one whole too (the
        // buffers end on a panel; what it reads past the packed records only reaches terms rows nobody
        // loads) — rocBLAS picks its kernel by the column count, and a chunk of 96 row-steps did not sum
        // like the 776 of the same call in one launch: with one shape for every call, a row-step's terms
        // are the same bits however the call is cut into launches
        const size_t cols_max = (size_t)(Lc_max + 1) * nb;
        const size_t cols_cap = kPanels ? (cols_max + kTermsPanel - 1) / kTermsPanel * kTermsPanel : cols_max;
        if (grow(h, h->d_X, h->X_cap, cols_cap * h->KXc) || grow(h, h->d_T, h->T_cap, cols_cap * N) ||
            grow(h, h->d_xstate, h->xstate_cap, (size_t)nb * kXcdWgs * state_w))
            return WRNN_EHIP;
        if (dbg_steps > 0 && !dbg.p) {
            dbg_G = nb * kXcdWgs;
            HIP_TRY(h, hipMalloc(&dbg.p, (size_t)dbg_G * dbg_steps * kStamps * 4));
            HIP_TRY(h, hipMemsetAsync(dbg.p, 0, (size_t)dbg_G * dbg_steps * kStamps * 4, st));
        }
        HIP_TRY(h, hipMemsetAsync(h->d_xgx, 0, (size_t)nb * kXXcdStride * 8, st));   // tags restart at 1
        for (int t0 = 0; t0 < L; t0 += Lc_max) {
            const int Lc = std::min(Lc_max, L - t0);
            const int rows = std::min(Lc + 1, L - t0);     // terms rows: steps [t0, t0 + rows)
            if (fs) {
                HIP_TRY(h, launch_terms_interp(h->d_FT, h->d_AT, fs->coef, h->d_T, N, fs->U, fs->NF, fs->NF + fs->nJ - 1,
                                               fs->hop, fs->nJ, fs->nf, fs->stride, fs->rb + b0, nb, t0, rows, st));
            } else {
                HIP_TRY(h, launch_pack_cond_input(cond, h->CD, B, b0, nb, t0, rows, h->KXc, h->d_X, st));
                const int cols = rows * nb, step = kPanels ? kTermsPanel : cols;
                for (int c0 = 0; c0 < cols; c0 += step)
                    if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, step, h->KXc,
                                      &one, h->d_xWt, h->KXc, h->d_X + (size_t)c0 * h->KXc, h->KXc, &zero,
                                      h->d_T + (size_t)c0 * N, N) != rocblas_status_success)
                        return fail(h, WRNN_EHIP, "rocblas_sgemm (conditioning terms) failed");
            }
            // the dense kernel's one-shot launches form no sampler draws: the terms the sampler adds, Philox
            // or injected, go into the padding of the chunk's terms rows and reach the loop with them
            if constexpr (std::is_same_v<Args, XcdArgs>)
                HIP_TRY(h, launch_xcd_draws(h->d_T, noise, seed, row_offset + b0, nb, B, b0, t0, rows, st));
            HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
            Args a{};
            a.slab = h->d_xslab;
            a.terms = h->d_T;
            a.noise = noise;
            a.out = out;
            a.state = h->d_xstate;
            a.xg = h->d_xgx;
            a.members = h->d_members;
            a.ctl = h->d_ctl;
            a.seed = seed;
            a.row0 = row_offset + b0;
            a.timeout_ticks = h->timeout_ticks;
            a.L = L;
            a.t0 = t0;
            a.Lc = Lc;
            a.Bt = B;
            a.b0 = b0;
            a.nb = nb;
            a.s = slab;
            a.dbg = (b0 == 0 && t0 == 0) ? dbg.p : nullptr;
            a.dbg_steps = std::min(dbg_steps, Lc);
            HIP_TRY(h, launch(a, st));
        }
    }
    if (dbg.p) return dump_stamps(h, dbg, (size_t)dbg_G * dbg_steps * kStamps, {dbg_G, dbg_steps, kStamps}, st);
    return WRNN_OK;
}

int generate_xcd(wrnn_t *h, const float *cond, const FrameSrc *fs, int B, int L, const float *noise, uint64_t seed,
                 int64_t row_offset, float *out, hipStream_t st) {
    return generate_xcd_rows<XcdArgs>(h, cond, fs, B, L, noise, seed, row_offset, out, st, kXTerms, kXStateW, h->xs,
                                      launch_xcd);
}

int generate_xcds(wrnn_t *h, const float *cond, const FrameSrc *fs, int B, int L, const float *noise, uint64_t seed,
                  int64_t row_offset, float *out, hipStream_t st) {
    return generate_xcd_rows<XcdsArgs>(h, cond, fs, B, L, noise, seed, row_offset, out, st, kSTerms, kSStateW, h->xss,
                                       launch_xcds);
}

// MoL rows through the XCD-resident many-row kernel: up to kMRowsMax rows per launch (launch row
// r on XCD r % 8, its row r / 8 there), time chunks sized so terms + GEMM input stay within
// WRNN_TERMS_MB (default 8192 MiB); the recurrent state is carried per workgroup in d_xmstate.
int generate_xcdm(wrnn_t *h, const float *cond, const FrameSrc *fs, int B, int L, const float *noise, uint64_t seed,
                  int64_t row_offset, float *out, int32_t *labels, hipStream_t st) {
    const int N = kXcdWgs * kMRing;   // compact terms record (d_xmWt)
    const bool raw = h->cfg.mode == WRNN_MODE_RAW;
    const int NK = raw ? kMRawNC : 11;              // draws per row-step: Exp(1) per class / MoL uniforms
    if (int rc = blas_on(h, st)) return rc;
    const double budget = terms_budget_floats();
    const size_t xg_words = (size_t)kXcds * kMXcdStride;
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    if (!h->d_xmxg) HIP_TRY(h, hipMalloc(&h->d_xmxg, xg_words * 8));
    if (!h->d_xmstate) HIP_TRY(h, hipMalloc(&h->d_xmstate, (size_t)kXcds * kXcdWgs * kMStateW * sizeof(float)));
    const int rows_max = kXcds * 4 * h->xcdm_nq;
    const float one = 1.0f, zero = 0.0f;
    XcdmGemm gemms[3];
    xcdm_terms_gemms(*h, gemms);
    // the segmented terms GEMMs writing C[m][N] for X [m][KXc]
    auto terms_gemm = [&](const float *X, int m, float *C) -> int {
        for (const XcdmGemm &g : gemms) {
            const rocblas_status rs =
                rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, g.rows, m, g.k, &one,
                              h->d_xmWt + (size_t)g.row0 * h->KXc + g.col0, h->KXc, X + g.col0, h->KXc, &zero,
                              C + g.row0, N);
            if (rs != rocblas_status_success) return fail(h, WRNN_EHIP, "rocblas_sgemm (conditioning terms) failed");
        }
        return WRNN_OK;
    };
    if (fs) {   // frame-rate terms (frame_terms.hip)
        if (int rc = frame_terms(h, *fs, N, h->KXc, h->cfg.feat_dims + h->cfg.aux_dims, st, terms_gemm)) return rc;
    }
    // diagnostics: WRNN_DEBUG_STAMPS=1 WRNN_DEBUG_FILE=<path>: per-wave phase stamps of the first
    // launch ([256 · kMWaves][kMDbgSteps][kMStamps] shader clocks, int32 header)
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = (!raw && dbg_env && std::atoi(dbg_env) > 0 && L >= kMDbgSkip + kMDbgSteps) ? kMDbgSteps : 0;
    const size_t dbg_n = (size_t)kXcds * kXcdWgs * kMWaves * dbg_steps * kMStamps;
    DbgBuf dbg;
    if (dbg_steps > 0) {
        HIP_TRY(h, hipMalloc(&dbg.p, dbg_n * 4));
        HIP_TRY(h, hipMemsetAsync(dbg.p, 0, dbg_n * 4, st));
    }
    for (int b0 = 0; b0 < B; b0 += rows_max) {
        const int nb = std::min(rows_max, B - b0);
        const int nq = (((nb + kXcds - 1) / kXcds) + 3) / 4;   // quads on the fullest XCD
        const int Lc_max = (int)std::max(1.0, std::min((double)L, budget / ((double)nb * (N + h->KXc + (noise ? 0 : NK)))));
        if (grow(h, h->d_X, h->X_cap, (size_t)Lc_max * nb * h->KXc) || grow(h, h->d_T, h->T_cap, (size_t)Lc_max * nb * N) ||
            (!noise && grow(h, h->d_xmnoise, h->xmnoise_cap, (size_t)Lc_max * nb * NK)))
            return WRNN_EHIP;
        // tags restart at 1, every packed hop element empty (fatchord_xcdm.h: all bits set)
        HIP_TRY(h, hipMemsetAsync(h->d_xmxg, 0xFF, xg_words * 8, st));
        for (int t0 = 0; t0 < L; t0 += Lc_max) {
            const int Lc = std::min(Lc_max, L - t0);
            if ((size_t)Lc * nb * h->KXc > h->X_cap || (size_t)Lc * nb * N > h->T_cap)
                return fail(h, WRNN_EINVAL, "xcdm: terms workspace too small");
            if (fs) {
                HIP_TRY(h, launch_terms_interp(h->d_FT, h->d_AT, fs->coef, h->d_T, N, fs->U, fs->NF, fs->NF + fs->nJ - 1,
                                               fs->hop, fs->nJ, fs->nf, fs->stride, fs->rb + b0, nb, t0, Lc, st));
            } else {
                HIP_TRY(h, launch_pack_cond_input(cond, h->CD, B, b0, nb, t0, Lc, h->KXc, h->d_X, st,
                                                  h->cfg.feat_dims + h->cfg.aux_dims));
                if (int rc = terms_gemm(h->d_X, Lc * nb, h->d_T)) return rc;
            }
            HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
            XcdmArgs a{};
            a.slab = h->d_xmslab;
            a.terms = h->d_T;
            if (noise) {   // injected [L][B][NK]
                a.noise = noise;
                a.nz_t0 = 0;
                a.nz_ts = B;
                a.nz_b0 = b0;
            } else {       // Philox, drawn for this chunk by a small kernel first ([Lc][nb][NK])
                HIP_TRY(h, launch_philox_fill(h->d_xmnoise, seed, row_offset + b0, nb, t0, Lc, NK, raw ? 0 : 1, st));
                a.noise = h->d_xmnoise;
                a.nz_t0 = t0;
                a.nz_ts = nb;
                a.nz_b0 = 0;
            }
            a.out = out;
            a.labels = labels;
            a.state = h->d_xmstate;
            a.xg = h->d_xmxg;
            a.members = h->d_members;
            a.ctl = h->d_ctl;
            a.seed = seed;
            a.row0 = row_offset + b0;
            a.timeout_ticks = h->timeout_ticks;
            a.L = L;
            a.t0 = t0;
            a.Lc = Lc;
            a.Bt = B;
            a.b0 = b0;
            a.nb = nb;
            a.s = h->xms;
            a.dbg = (b0 == 0 && t0 == 0 && Lc >= kMDbgSkip + kMDbgSteps) ? dbg.p : nullptr;
            HIP_TRY(h, launch_xcdm(a, nq, raw, st));
        }
    }
    if (dbg.p) return dump_stamps(h, dbg, dbg_n, {kXcds * kXcdWgs * kMWaves, dbg_steps, kMStamps}, st);
    return WRNN_OK;
}

int generate_latency(wrnn_t *h, const float *cond, int B, int L, const float *noise, uint64_t seed,
                     int64_t row_offset, float *out, int32_t *labels, hipStream_t st) {
    const wrnn_config &c = h->cfg;
    const int R = c.rnn_dims;
    const int Bc_max = std::min(B, h->max_rows);
    // workspaces (grow-only)
    if (grow(h, h->d_cI, h->cI_cap, (size_t)L * Bc_max * R)) return WRNN_EHIP;
    // hand-off replicas (WRNN_REPLICAS, default 8), each padded to a 64 KiB boundary; at most
    // 64 / kTermsPerUnit, since one wave publishes every term of a unit to every replica at once
    // (8 measured best: 8.18 us/step at rnn 512 B=1; 4 -> 8.27, 16 -> 8.77, 2 -> 8.84)
    const char *rep_env = std::getenv("WRNN_REPLICAS");
    const int reps = std::max(1, std::min(64 / kTermsPerUnit, rep_env ? std::atoi(rep_env) : 8));
    // replica stride ≥ 64 KiB: keeps replicas on different lines/channels and makes the
    // pollers' fixed-count over-reads (slots ≥ n) land in allocated memory
    const long long vec_max = std::max<long long>({(long long)Bc_max * h->NMAX, (long long)Bc_max * R * kTermsPerUnit,
                                                   3LL * R});
    const long long rep_stride = (((vec_max + kOverRead) * 8 + 65535) / 65536) * 65536 / 8;
    const size_t need_xg = (size_t)kHops * reps * rep_stride;
    HIP_TRY(h, ensure(h->d_xg, h->xg_cap, need_xg));
    // diagnostics: WRNN_DEBUG_STAMPS=<steps> WRNN_DEBUG_FILE=<path> dumps per-stage stamps
    const char *dbg_env = std::getenv("WRNN_DEBUG_STAMPS");
    const int dbg_steps = dbg_env ? std::min(L, std::atoi(dbg_env)) : 0;
    DbgBuf dbg;
    if (dbg_steps > 0) {
        HIP_TRY(h, hipMalloc(&dbg.p, (size_t)h->G * dbg_steps * kStamps * 4));
        HIP_TRY(h, hipMemsetAsync(dbg.p, 0, (size_t)h->G * dbg_steps * kStamps * 4, st));
    }
    for (int b0 = 0; b0 < B; b0 += h->max_rows) {
        const int Bc = std::min(h->max_rows, B - b0);
        HIP_TRY(h, launch_ci_gemm(cond, h->CD, B, b0, Bc, 0, L, h->d_IW, 1 + c.feat_dims + c.aux_dims, h->d_Ib, R,
                                  c.feat_dims + c.aux_dims, h->d_cI, R, st));
        HIP_TRY(h, hipMemsetAsync(h->d_xg, 0, need_xg * 8, st));
        LoopArgs a{};
        a.slab = h->d_slab;
        a.cI = h->d_cI;
        a.cond = cond;
        a.noise = noise;
        a.out = out;
        a.labels = labels;
        a.xg = h->d_xg;
        a.reps = reps;
        {
            const char *dp = std::getenv("WRNN_DELAY_POLL");
            a.delay_poll = dp ? std::atoi(dp) : 1;
        }
        a.rep_stride = rep_stride;
        a.ctl = h->d_ctl;
        a.seed = seed;
        a.row0 = row_offset + b0;
        a.timeout_ticks = h->timeout_ticks;
        a.L = L;
        a.Bc = Bc;
        a.Bt = B;
        a.b0 = b0;
        a.R = R;
        a.F = c.fc_dims;
        a.A = c.aux_dims;
        a.CD = h->CD;
        a.feat = c.feat_dims;
        a.NC = c.n_classes;
        a.NK = h->NK;
        a.mol = c.mode == WRNN_MODE_MOL;
        a.U = h->U;
        a.UF = h->UF;
        a.UC = h->UC;
        a.G = h->G;
        a.NMAX = h->NMAX;
        a.s = h->s;
        a.dbg = (b0 == 0) ? dbg.p : nullptr;
        a.dbg_steps = dbg_steps;
        HIP_TRY(h, launch_loop(a, lds_bytes_for(*h, Bc), st));
    }
    if (dbg.p) return dump_stamps(h, dbg, (size_t)h->G * dbg_steps * kStamps, {h->G, dbg_steps, kStamps}, st);
    return WRNN_OK;
}

}  // namespace

namespace wrnn {
namespace host {

double terms_budget_floats() {
    const char *mb_env = std::getenv("WRNN_TERMS_MB");
    return (mb_env ? std::atof(mb_env) : 8192.0) * (1 << 20) / 4.0;
}

// ---- the multi-row kernel's launch loop in pieces (generate_rows; the rows sessions of capi_stream.cpp)
bool rows_grouped(const wrnn_ctx &h, int B) {
    const char *grp_env = std::getenv("WRNN_ROW_GROUPS");
    const int grp_force = grp_env ? std::atoi(grp_env) : 0;
    const bool can_group = h.g2.ok && !h.sparse && grp_force != 1;
    return can_group && B >= 2 && (grp_force == 2 || std::min(B, kRowsMax) >= kGroupRows);
}

int rows_hop_areas(wrnn_t *h) {
    const size_t flag_words = (size_t)kRowsHops * kFlagSlots * kFlagStride, xr_words = (size_t)kXReps * kXRepStride;
    if (!h->d_flags) {
        HIP_TRY(h, hipMalloc(&h->d_flags, 2 * flag_words * 4));
        HIP_TRY(h, hipMalloc(&h->d_xr, 2 * xr_words * 8));
    }
    return WRNN_OK;
}

int rows_block(wrnn_t *h, bool grouped, int rows_left, int steps, RowsBlock *out) {
    const wrnn_config &c = h->cfg;
    const char *gran_env = std::getenv("WRNN_ROWS_GRANULES");
    const int gran_force = gran_env ? std::atoi(gran_env) : -1;
    RowsBlock k{};
    k.ng = grouped ? 2 : 1;
    const int ng = k.ng;
    k.N = h->rG * h->NT;
    int Bl = std::min(rows_left, kRowsMax);
    auto group_rows = [&](int bl, int g) { const int b_0 = (bl + ng - 1) / ng; return g == 0 ? b_0 : bl - b_0; };
    while (Bl > 1 && rows_tile_for(*h, group_rows(Bl, 0)) == 0 && rows_tile_for(*h, group_rows(Bl, 0), false) == 0) --Bl;
    // two groups: never leave one row for the next block (its second group would have no rows: a launch of
    // no blocks for its terms and G/2 workgroups looping over nothing), 257 rows are 255 + 2
    if (ng == 2 && rows_left - Bl == 1 && Bl > 2) --Bl;
    const int Bg = group_rows(Bl, 0);          // rows of group 0 (>= those of group 1)
    k.Bl = Bl;
    k.Bg = Bg;
    k.Bg1 = group_rows(Bl, 1);
    // the MoL head stays in LDS while all rows fit one tile next to it; beyond that, larger
    // tiles are worth more than an LDS-resident head (the samplers then read it from L2)
    k.mol = c.mode == WRNN_MODE_MOL;
    const int tb_in = rows_tile_for(*h, Bg);
    k.head_lds = !k.mol || tb_in >= std::min(Bg, 16) || rows_tile_for(*h, Bg, false) == 0;
    k.TB = k.head_lds ? tb_in : rows_tile_for(*h, Bg, false);
    if (k.TB == 0) return fail(h, WRNN_EUNSUPPORTED, "rows kernel: one row of state does not fit LDS");
    k.SW = rows_state_width(h->rU, h->rUF);
    // GEMM input width: the composed MoL record (KXc = CD + 4) or [cI | a2 a3 a4 | 1 0 0 0]
    // (KX); either may be the larger one (tiny dims: KXc 100 > KX 80)
    k.KXg = rows_terms_kx(*h);
    k.Lc_max = (int)std::max(1.0, std::min((double)steps, terms_budget_floats() / ((double)Bl * (k.N + k.KXg))));
    k.T_grp = (size_t)k.Lc_max * Bg * k.N;
    k.act_grp = (size_t)kRowsHops * 2 * Bg * h->KA;
    k.state_grp = (size_t)h->rG * Bg * k.SW + Bg;
    // granule hand-offs while a group's hop vector is small (kRowsGranMax values; measured
    // crossover); WRNN_ROWS_GRANULES=0|1 forces bulk / granules.
    k.gran = gran_force == 1 || (gran_force != 0 && (size_t)Bg * h->KA <= kRowsGranMax);
    k.gstride = (((long long)Bg * h->KA + kRowsGranPad + 15) / 16) * 16;
    // bulk mode, MoL: the f2 hop alone as granules (one hop region per group)
    k.f2g = !k.gran && k.mol;
    *out = k;
    return WRNN_OK;
}

// The flags, x granules and hop granules of the block's groups zeroed: tags restart at 1 with every
// generate() (and no tag of an earlier call can satisfy a poll of a session's push).  `act`: the bulk
// activation matrices too.
int rows_reset(wrnn_t *h, const RowsBlock &k, bool act, hipStream_t st) {
    const size_t flag_words = (size_t)kRowsHops * kFlagSlots * kFlagStride, xr_words = (size_t)kXReps * kXRepStride;
    HIP_TRY(h, hipMemsetAsync(h->d_flags, 0, k.ng * flag_words * 4, st));
    HIP_TRY(h, hipMemsetAsync(h->d_xr, 0, k.ng * xr_words * 8, st));
    if (k.gran || k.f2g) {
        const size_t n = (size_t)k.ng * (k.gran ? kRowsHops : 1) * k.gstride;
        HIP_TRY(h, ensure(h->d_gact, h->gact_cap, n));
        HIP_TRY(h, hipMemsetAsync(h->d_gact, 0, n * 8, st));
    }
    if (act) HIP_TRY(h, hipMemsetAsync(h->d_act, 0, k.ng * k.act_grp * sizeof(float), st));
    return WRNN_OK;
}

// Steps [t0, t0 + Lc) of the block: the conditioning terms per group (cI or the composed record, then
// one fp32 GEMM for every workgroup's terms) and one persistent launch.  The workspaces are grown.
int rows_chunk(wrnn_t *h, const RowsBlock &k, const RowsRun &r, int t0, int Lc, hipStream_t st) {
    const wrnn_config &c = h->cfg;
    const int R = c.rnn_dims, A = c.aux_dims, N = k.N, KXg = k.KXg, Bg = k.Bg;
    const size_t flag_words = (size_t)kRowsHops * kFlagSlots * kFlagStride, xr_words = (size_t)kXReps * kXRepStride;
    const float one = 1.0f, zero = 0.0f;
    const bool grouped = k.ng == 2;
    const int tc = t0 - r.cond_t0;              // the chunk's first record in cond
    for (int g = 0; g < k.ng; ++g) {
        const int bg0 = r.b0 + (g ? Bg : 0), nb = g ? k.Bg1 : Bg;
        if ((size_t)Lc * nb * KXg > h->X_cap) return fail(h, WRNN_EINVAL, "terms-GEMM input exceeds its workspace");
        if (rows_terms_composed(*h)) {
            HIP_TRY(h, launch_pack_cond_input(r.cond, h->CD, r.Bt, bg0, nb, tc, Lc, KXg, h->d_X, st));
        } else {
            HIP_TRY(h, launch_ci_gemm(r.cond, h->CD, r.Bt, bg0, nb, tc, Lc, h->d_IW, 1 + c.feat_dims + A, h->d_Ib, R,
                                      c.feat_dims + A, h->d_X, h->KX, st));
            HIP_TRY(h, launch_pack_terms_input(r.cond, h->CD, r.Bt, bg0, nb, tc, Lc, c.feat_dims, A, R, h->KX, h->d_X, st));
        }
        if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, Lc * nb, KXg, &one,
                          h->d_Wt, KXg, h->d_X, KXg, &zero, h->d_T + g * k.T_grp, N) != rocblas_status_success)
            return fail(h, WRNN_EHIP, "rocblas_sgemm (conditioning terms) failed");
    }
    RowsArgs a{};
    a.slab = h->d_rslab;
    a.terms = h->d_T;
    a.noise = r.noise;
    a.out = r.out;
    a.labels = r.labels;
    a.act = h->d_act;
    a.flags = h->d_flags;
    a.xg = h->d_xr;
    a.gact = k.gran ? h->d_gact : nullptr;
    a.gstride = k.gstride;
    a.gf2 = k.f2g ? h->d_gact : nullptr;
    a.state = r.state;
    a.ctl = h->d_ctl;
    a.seed = r.seed;
    a.row0 = r.row_offset + r.b0;
    a.timeout_ticks = h->timeout_ticks;
    a.L = r.out_ld;
    a.t0 = t0;
    a.Lc = Lc;
    a.B = Bg;
    a.Bt = r.Bt;
    a.b0 = r.b0;
    a.R = R;
    a.F = c.fc_dims;
    a.A = A;
    a.NC = c.n_classes;
    a.NK = h->NK;
    a.mol = c.mode == WRNN_MODE_MOL;
    a.U = h->rU;
    a.UF = h->rUF;
    a.UC = h->rUC;
    a.G = h->rG;
    a.NT = h->NT;
    a.TB = k.TB;
    a.KA = h->KA;
    a.s = h->rs;
    a.dbg = r.dbg;
    a.dbg_steps = r.dbg_steps;
    a.head_lds = k.head_lds ? 1 : 0;
    a.gw = h->rows_gw ? 1 : 0;
    RowsGroup g1{};
    if (grouped) {
        g1.terms = h->d_T + k.T_grp;
        g1.act = h->d_act + k.act_grp;
        g1.flags = h->d_flags + flag_words;
        g1.xg = h->d_xr + xr_words;
        g1.gact = k.gran ? h->d_gact + (size_t)kRowsHops * k.gstride : nullptr;
        g1.gf2 = k.f2g ? h->d_gact + k.gstride : nullptr;
        g1.state = r.state + k.state_grp;
        g1.row0 = r.row_offset + r.b0 + Bg;
        g1.B = k.Bg1;
        g1.b0 = r.b0 + Bg;
        g1.dbg = nullptr;
    }
    HIP_TRY(h, launch_rows(a, grouped ? &g1 : nullptr, rows_lds_bytes(*h, Bg, k.TB, k.head_lds), st));
    return WRNN_OK;
}

int blas_on(wrnn_t *h, hipStream_t st) {
    if (!h->blas && rocblas_create_handle(&h->blas) != rocblas_status_success)
        return fail(h, WRNN_EHIP, "rocblas_create_handle failed");
    if (rocblas_set_stream(h->blas, st) != rocblas_status_success) return fail(h, WRNN_EHIP, "rocblas_set_stream failed");
    return WRNN_OK;
}

int upload_coef(wrnn_t *h, const std::vector<float> &coef, hipStream_t st) {
    if (coef == h->coef_host) return WRNN_OK;
    if (grow(h, h->d_coef, h->coef_cap, coef.size())) return WRNN_EHIP;
    HIP_TRY(h, hipMemcpyAsync(h->d_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));   // the caller's `coef` may be a local: the copy completes before it goes
    h->coef_host = coef;
    return WRNN_OK;
}

// The UpsampleNetwork's frame weights (fatchord_version.py:64-89): the response κ of pad →
// Stretch2d(s_i) → Conv2d(1, 2s_i+1, pad s_i) (×n) to one unit frame, in float64, as
// coef[φ][k] = κ(φ − hop·(k + jlo)).  Each stage spreads a frame by ±s_i samples at its rate,
// E = Σ s_i·hop / r_i samples at the output rate (r_i = s_1···s_i): κ lives on [−E, hop − 1 + E].
// Exact (equal to the stage-wise zero-padded cascade over the cropped output) when the pad
// frames cover that reach: pad·hop ≥ E.  Returns false otherwise (the caller keeps the
// per-sample conditioning path).
bool frame_weights(const wrnn_upsample_cfg &c, int *hop_out, int *nJ_out, int *jlo_out, std::vector<float> &coef) {
    int hop = 1;
    for (int i = 0; i < c.n_scales; ++i) hop *= c.scales[i];
    long long E = 0;
    for (int i = 0, r = 1; i < c.n_scales; ++i) {
        r *= c.scales[i];
        E += (long long)c.scales[i] * (hop / r);
    }
    if ((long long)c.pad * hop < E) return false;
    const int jlo = -(int)((hop - 1 + E) / hop), jhi = (int)((E + hop - 1) / hop);
    const int nJ = jhi - jlo + 1;
    if (nJ > 8) return false;
    // unit frame at index W of 2W + 1 frames, W beyond the reach
    const int W = jhi - jlo + 1;
    std::vector<double> x(2 * W + 1, 0.0);
    x[W] = 1.0;
    for (int i = 0; i < c.n_scales; ++i) {
        const int s = c.scales[i];
        std::vector<double> y(x.size() * s), z(x.size() * s, 0.0);
        for (size_t n = 0; n < y.size(); ++n) y[n] = x[n / s];
        for (long long n = 0; n < (long long)z.size(); ++n) {
            double acc = 0.0;
            for (int m = 0; m <= 2 * s; ++m) {
                const long long q = n + m - s;
                if (q >= 0 && q < (long long)y.size()) acc += (double)c.taps[i][m] * y[q];
            }
            z[n] = acc;
        }
        x.swap(z);
    }
    coef.assign((size_t)hop * nJ, 0.0f);
    for (int ph = 0; ph < hop; ++ph)
        for (int k = 0; k < nJ; ++k) {
            const long long d = ph - (long long)hop * (k + jlo);   // output offset from the frame's first sample
            const long long n = d + (long long)W * hop;
            if (n >= 0 && n < (long long)x.size()) coef[(size_t)ph * nJ + k] = (float)x[n];
        }
    *hop_out = hop;
    *nJ_out = nJ;
    *jlo_out = jlo;
    return true;
}

int check_upsample_dims(wrnn_t *h, const wrnn_upsample_cfg *ucfg) {
    if (ucfg->feat_dims != h->cfg.feat_dims || ucfg->res_out_dims != h->CD - h->cfg.feat_dims)
        return fail(h, WRNN_EINVAL, "upsample config does not match the handle's feat / aux dims");
    return WRNN_OK;
}

int check_upsample_scales(wrnn_t *h, const wrnn_upsample_cfg *ucfg) {
    if (ucfg->n_scales < 1 || ucfg->n_scales > 4) return fail(h, WRNN_EINVAL, "1..4 upsample scales");
    for (int i = 0; i < ucfg->n_scales; ++i)
        if (ucfg->scales[i] < 1 || !ucfg->taps[i]) return fail(h, WRNN_EINVAL, "bad upsample scale / taps");
    return WRNN_OK;
}

int frame_form(wrnn_t *h, const wrnn_upsample_cfg *ucfg, int *hop, int *nJ, int *jlo, std::vector<float> &coef) {
    if (!frame_weights(*ucfg, hop, nJ, jlo, coef))
        return fail(h, WRNN_EUNSUPPORTED,
                    "the upsample cascade has no exact frame-rate form (pad frames < its reach, or more than 8 taps)");
    return WRNN_OK;
}

constexpr int kXcdDefaultRows = 48;
constexpr int kXcdmMinRows = 9;

LoopPath choose_path(const wrnn_t *h, int B) {
    const char *path_env = std::getenv("WRNN_PATH");
    const std::string pe = path_env ? path_env : "";
    // deepmind hidden 896 / quantisation 256: the XCD-resident kernel (WRNN_PATH=rows: the multi-row one)
    if (h->dm) return h->dx_ok && pe != "rows" ? P_DX : P_DM;
    bool rows = h->max_rows < 1 || B > h->max_rows;
    if (pe == "rows") rows = true;
    if (pe == "latency" && h->max_rows >= 1) rows = false;
    if (rows && !h->rows_ok) rows = false;
    // MoL rnn / fc 512 up to kXcdDefaultRows rows: the XCD-resident kernel (8 rows per launch;
    // beyond that the multi-row kernel's throughput wins)
    // MoL rnn / fc 512, more than kXcdmMinRows rows: the many-row XCD-resident kernel (MFMA)
    // (RAW 512-class: the many-row kernel for every row count — it is the only XCD-resident RAW one)
    if (h->xcdm_ok && (pe == "xcdm" || (pe.empty() && (B >= kXcdmMinRows || h->cfg.mode == WRNN_MODE_RAW))))
        return P_XCDM;
    if (h->xcd_ok && (pe == "xcd" || (pe.empty() && B <= kXcdDefaultRows))) return P_XCD;
    // MoL rnn 896 with block-sparse GRU weights likewise: the XCD-resident sparse kernel
    if (h->xcds_ok && (pe == "xcd" || (pe.empty() && B <= kXcdDefaultRows))) return P_XCDS;
    if (h->split_ok && (pe == "split" || (pe.empty() && B == 1))) return P_SPLIT;
    return rows ? P_ROWS : P_LATENCY;
}

}  // namespace host
}  // namespace wrnn

// One loop run over the chosen path, between the two timing events.  `fs` (frame-rate terms)
// only for the XCD-resident paths.
static int run_loop(wrnn_t *h, LoopPath path, const float *cond, const FrameSrc *fs, int B, int L, const float *noise,
             uint64_t seed, int64_t row_offset, float *out, int32_t *labels, hipStream_t st) {
    HIP_TRY(h, hipMemsetAsync(h->d_ctl, 0, kCtlWords * sizeof(int), st));
    HIP_TRY(h, hipEventRecord(h->ev0, st));
    set_last_path(h, path == P_ROWS && h->rows_gw ? 9 : path == P_DM && h->dm_gw ? 10 : (int)path);
    int rc = WRNN_OK;
    switch (path) {
        case P_DX: rc = generate_dx(h, B, L, noise, seed, row_offset, out, labels, st); break;
        case P_DM: rc = generate_dm(h, B, L, noise, seed, row_offset, out, labels, st); break;
        case P_XCDM: rc = generate_xcdm(h, cond, fs, B, L, noise, seed, row_offset, out, labels, st); break;
        case P_XCD: rc = generate_xcd(h, cond, fs, B, L, noise, seed, row_offset, out, st); break;
        case P_XCDS: rc = generate_xcds(h, cond, fs, B, L, noise, seed, row_offset, out, st); break;
        case P_SPLIT: rc = generate_split(h, cond, B, L, noise, seed, row_offset, out, st); break;
        case P_ROWS: rc = generate_rows(h, cond, B, L, noise, seed, row_offset, out, labels, st); break;
        default: rc = generate_latency(h, cond, B, L, noise, seed, row_offset, out, labels, st); break;
    }
    if (rc != WRNN_OK) return rc;
    HIP_TRY(h, hipEventRecord(h->ev1, st));
    h->timed = true;
    return WRNN_OK;
}

int wrnn_generate(wrnn_t *h, const float *cond, int B, int L, const float *noise, uint64_t seed,
                  int64_t row_offset, float *out, int32_t *labels, void *stream) {
    if (!h) return WRNN_EINVAL;
    if (!h->ready) return fail(h, WRNN_ENOWEIGHTS, "weights not (fully) set");
    if (B <= 0 || L <= 0 || !out || (!cond && !h->dm)) return fail(h, WRNN_EINVAL, "need B > 0, L > 0, cond and out");
    if (labels && h->cfg.mode == WRNN_MODE_MOL) return fail(h, WRNN_EINVAL, "labels are a RAW / DM output");
    HIP_TRY(h, hipSetDevice(h->device));
    return run_loop(h, choose_path(h, B), cond, nullptr, B, L, noise, seed, row_offset, out, labels,
                    (hipStream_t)stream);
}

int wrnn_frame_weights(const wrnn_upsample_cfg *ucfg, int *hop, int *nJ, int *jlo, float *coef, int coef_cap) {
    if (!ucfg) return WRNN_EINVAL;
    if (int rc = check_upsample_scales(nullptr, ucfg)) return rc;
    int hh = 1, nj = 1, jl = 0;
    std::vector<float> c;
    if (int rc = frame_form(nullptr, ucfg, &hh, &nj, &jl, c)) return rc;
    if (hop) *hop = hh;
    if (nJ) *nJ = nj;
    if (jlo) *jlo = jl;
    if (coef) {
        if (coef_cap < (int)c.size()) return WRNN_EINVAL;
        std::memcpy(coef, c.data(), c.size() * sizeof(float));
    }
    return WRNN_OK;
}

int wrnn_generate_frames(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *mel, const float *aux, int U, int T,
                         int target, int overlap, const float *noise, uint64_t seed, int64_t row_offset, float *out,
                         int32_t *labels, void *stream) {
    return wrnn_generate_frames_rows(h, ucfg, mel, aux, U, T, target, overlap, 0, -1, noise, seed, row_offset, out,
                                     labels, stream);
}

// row_count < 0: every row of the launch (wrnn_generate_frames)
int wrnn_generate_frames_rows(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *mel, const float *aux, int U,
                              int T, int target, int overlap, int row_begin, int row_count, const float *noise,
                              uint64_t seed, int64_t row_offset, float *out, int32_t *labels, void *stream) {
    if (!h) return WRNN_EINVAL;
    if (!h->ready) return fail(h, WRNN_ENOWEIGHTS, "weights not (fully) set");
    if (h->dm) return fail(h, WRNN_EINVAL, "deepmind handles take no conditioning (wrnn_generate)");
    if (!ucfg || !mel || !out || U <= 0 || T <= 0) return fail(h, WRNN_EINVAL, "need ucfg, mel, out, U > 0, T > 0");
    if (labels && h->cfg.mode == WRNN_MODE_MOL) return fail(h, WRNN_EINVAL, "labels are a RAW / DM output");
    // (the scales are wrnn_cond_shape's to refuse, with its text)
    if (int rc = check_upsample_dims(h, ucfg)) return rc;
    if (ucfg->res_out_dims > 0 && !aux) return fail(h, WRNN_EINVAL, "need aux (MelResNet output)");
    int L = 0, Ball = 0;
    if (int rc = wrnn_cond_shape(ucfg, U, T, target, overlap, &L, &Ball))
        return fail(h, rc, std::string("conditioning shape: ") + wrnn_cond_last_error());
    if (row_count < 0) {
        row_begin = 0;
        row_count = Ball;
    }
    if (row_begin < 0 || row_count < 1 || row_begin + row_count > Ball)
        return fail(h, WRNN_EINVAL, "rows [row_begin, row_begin + row_count) outside the launch's " + std::to_string(Ball));
    const int B = row_count;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const LoopPath path = choose_path(h, B);
    FrameSrc fs;
    std::vector<float> coef;
    bool frames = (path == P_XCD || path == P_XCDS || path == P_XCDM) && std::getenv("WRNN_NO_FRAME_TERMS") == nullptr &&
                  frame_weights(*ucfg, &fs.hop, &fs.nJ, &fs.jlo, coef);
    if (frames) {
        const int N = kXcdWgs * (path == P_XCD ? kXTerms : path == P_XCDS ? kSTerms : kMRing);
        frames = N % 4 == 0;
    }
    if (!frames) {   // the per-sample conditioning (wrnn_upsample_pack) into a handle workspace
        const size_t rec = (size_t)h->CD * sizeof(float);
        if (grow(h, h->d_cond, h->cond_cap, (size_t)L * (Ball + (B < Ball ? B : 0)) * h->CD)) return WRNN_EHIP;
        if (int rc = wrnn_upsample_pack(ucfg, mel, aux, U, T, target, overlap, h->d_cond, stream))
            return fail(h, rc, std::string("upsample_pack: ") + wrnn_cond_last_error());
        const float *cond = h->d_cond;
        if (B < Ball) {   // the rows' records, compacted after the launch's [L][Ball] block
            float *sub = h->d_cond + (size_t)L * Ball * h->CD;
            HIP_TRY(h, hipMemcpy2DAsync(sub, B * rec, h->d_cond + (size_t)row_begin * h->CD, Ball * rec, B * rec, L,
                                        hipMemcpyDeviceToDevice, st));
            cond = sub;
        }
        return run_loop(h, path, cond, nullptr, B, L, noise, seed, row_offset, out, labels, st);
    }
    if (int rc = upload_coef(h, coef, st)) return rc;
    fs.mel = mel;
    fs.aux = aux;
    fs.U = U;
    fs.NF = T;
    fs.nf = Ball / U;
    fs.rb = row_begin;
    fs.stride = target > 0 ? target + overlap : 0;
    fs.coef = h->d_coef;
    return run_loop(h, path, nullptr, &fs, B, L, noise, seed, row_offset, out, labels, st);
}
