// capi_lists.cpp — list calls of the C-ABI host: the lane list on the one-row XCD kernels, the wide
// list and the folded list on the many-row kernel's grouped launches, and their host-only planners.
#include "host_ctx.h"

using namespace wrnn;
using namespace wrnn::host;

// ---- lists (wavernn_amd.h: wrnn_list_plan, wrnn_generate_list) ------------------------------
// Longest-processing-time-first over `lanes` lanes: utterances by decreasing length (ties: lower
// index first), each to the lane with the smallest load so far (ties: lowest lane); a lane runs
// its utterances in the order they were assigned.
static void list_plan(const int *frames, int U, int lanes, int *lane_of, int *pos_in_lane, int64_t *lane_len,
                      std::vector<int> *queue = nullptr) {   // queue [lanes]: the lanes' utterances in running order
    std::vector<int> order(U);
    for (int i = 0; i < U; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return frames[x] > frames[y]; });
    std::vector<int> count(lanes, 0);
    for (int k = 0; k < lanes; ++k) lane_len[k] = 0;
    for (int i : order) {
        int best = 0;
        for (int k = 1; k < lanes; ++k)
            if (lane_len[k] < lane_len[best]) best = k;
        lane_of[i] = best;
        pos_in_lane[i] = count[best]++;
        lane_len[best] += frames[i];
        if (queue) queue[best].push_back(i);
    }
}

// The upsample side of every list call: the config matches the handle, aux is there when the model
// has aux dims, and the cascade has an exact frame-rate form → hop, nJ, jlo and the frame weights.
static int list_upsample(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *aux, int *hop, int *nJ, int *jlo,
                         std::vector<float> &coef) {
    if (int rc = check_upsample_dims(h, ucfg)) return rc;
    if (int rc = check_upsample_scales(h, ucfg)) return rc;
    if (h->CD - h->cfg.feat_dims > 0 && !aux) return fail(h, WRNN_EINVAL, "need aux (MelResNet outputs)");
    return frame_form(h, ucfg, hop, nJ, jlo, coef);
}

// The arena of a list call: utterance i's frame-term stores FT [T_i + nJ − 1][N] at ft[i] and
// AT [T_i + 1][N] at at[i] (floats into d_larena), one utterance after the other.
struct ListArena {
    std::vector<size_t> ft, at;
    size_t total = 0;
    int Tmax = 0, nJ = 1;
    ListArena() = default;
    ListArena(const int *T, int U, int nJ_, int N) : ft(U), at(U), nJ(nJ_) {
        for (int i = 0; i < U; ++i) {
            ft[i] = total;
            total += (size_t)(T[i] + nJ - 1) * N;
            at[i] = total;
            total += (size_t)(T[i] + 1) * N;
            Tmax = std::max(Tmax, T[i]);
        }
    }
    // the arena, and the frame records and GEMM input of the longest utterance (frame_terms then grows nothing)
    int reserve(wrnn_t *h) const {
        const int fmax = std::max(Tmax + nJ - 1, Tmax + 1);
        return grow(h, h->d_frec, h->frec_cap, (size_t)fmax * h->CD) || grow(h, h->d_X, h->X_cap, (size_t)fmax * h->KXc) ||
               grow(h, h->d_larena, h->larena_cap, total);
    }
};

// Each utterance's frame-term stores in the arena through gemm (frame_terms), with the launches and
// shapes of its own wrnn_generate_frames call: rocBLAS picks its tiling by shape, so one GEMM over
// several utterances would move the last bit.
template <typename Gemm>
static int list_frame_terms(wrnn_t *h, const float *const *mel, const float *const *aux, const int *T, int U, int hop,
                            int nJ, int jlo, const ListArena &arena, int N, int split, hipStream_t st, Gemm gemm) {
    for (int i = 0; i < U; ++i) {
        FrameSrc fs;
        fs.mel = mel[i];
        fs.aux = aux ? aux[i] : nullptr;
        fs.U = 1;
        fs.NF = T[i];
        fs.hop = hop, fs.nJ = nJ, fs.jlo = jlo;
        fs.coef = h->d_coef;
        if (int rc = frame_terms(h, fs, N, h->KXc, split, st, gemm, h->d_larena + arena.ft[i], h->d_larena + arena.at[i]))
            return rc;
    }
    return WRNN_OK;
}

int wrnn_list_plan(const int *frames, int U, int lanes, int *lane_of, int *pos_in_lane, int64_t *lane_frames) {
    if (!frames || !lane_of || !pos_in_lane || !lane_frames) return cond_fail(WRNN_EINVAL, "need frames, lane_of, pos_in_lane and lane_frames");
    if (U < 1) return cond_fail(WRNN_EINVAL, "a list has at least one utterance");
    if (lanes < 1 || lanes > kXcds) return cond_fail(WRNN_EINVAL, "lanes is 1.." + std::to_string(kXcds));
    for (int i = 0; i < U; ++i)
        if (frames[i] < 21)
            return cond_fail(WRNN_EINVAL, "utterance " + std::to_string(i) + " has " + std::to_string(frames[i]) +
                                              " frames: fewer than 21 (the fade-out, as wrnn_postprocess)");
    list_plan(frames, U, lanes, lane_of, pos_in_lane, lane_frames);
    return WRNN_OK;
}

int wrnn_generate_list(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                       const int *T, int U, int lanes, const float *const *noise, uint64_t seed, int64_t row_offset,
                       float *const *out, void *stream) {
    if (!h) return WRNN_EINVAL;
    if (!h->ready) return fail(h, WRNN_ENOWEIGHTS, "weights not (fully) set");
    // ---- every argument of every utterance, before anything is queued or any workspace touched
    if (!ucfg || !mel || !T || !out || U < 1) return fail(h, WRNN_EINVAL, "need ucfg, mel, T, out and U >= 1");
    if (lanes < 1 || lanes > kXcds) return fail(h, WRNN_EINVAL, "lanes is 1.." + std::to_string(kXcds) + " (one per XCD)");
    if (h->dm || h->cfg.mode != WRNN_MODE_MOL)
        return fail(h, WRNN_EUNSUPPORTED, "lists run the one-row XCD MoL kernels: this handle is not MoL");
    const LoopPath path = choose_path(h, lanes);
    if (path != P_XCD && path != P_XCDS)
        return fail(h, WRNN_EUNSUPPORTED,
                    "lists run the dense rnn/fc 512 XCD kernel or the block-sparse rnn 896 one; " + std::to_string(lanes) +
                        " row(s) of this handle take loop path " + std::to_string((int)path));
    const int A4 = h->CD - h->cfg.feat_dims;
    int hop = 1, nJ = 1, jlo = 0;
    std::vector<float> coef;
    if (int rc = list_upsample(h, ucfg, aux, &hop, &nJ, &jlo, coef)) return rc;
    const int N = kXcdWgs * (path == P_XCD ? kXTerms : kSTerms), state_w = path == P_XCD ? kXStateW : kSStateW;
    for (int i = 0; i < U; ++i) {
        const std::string who = "utterance " + std::to_string(i);
        if (T[i] < 21) return fail(h, WRNN_EINVAL, who + " has " + std::to_string(T[i]) + " frames: fewer than 21 (the fade-out, as wrnn_postprocess)");
        if ((long long)T[i] * hop > INT_MAX) return fail(h, WRNN_EINVAL, who + ": hop * frames exceeds the step counter");
        if (!mel[i] || !out[i] || (A4 > 0 && !aux[i])) return fail(h, WRNN_EINVAL, who + ": need mel, aux and out");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;

    // ---- the schedule: lanes, then rounds of C lane-steps cut into pieces at utterance boundaries
    std::vector<int> lane_of(U), pos(U);
    int64_t lane_frames[kXcds];
    std::vector<std::vector<int>> queue(lanes);
    list_plan(T, U, lanes, lane_of.data(), pos.data(), lane_frames, queue.data());
    long long longest = 0;
    for (int k = 0; k < lanes; ++k) longest = std::max(longest, (long long)lane_frames[k] * hop);
    const double budget = terms_budget_floats();
    const long long C = (long long)std::max(1.0, std::min((double)longest, std::floor(budget / ((double)lanes * N) - 1.0)));
    const int rounds = (int)((longest + C - 1) / C);
    struct Piece {
        int u, t0, Lc, nt;
    };
    std::vector<Piece> pcs;
    std::vector<int> first((size_t)rounds * (kXcds + 1), 0);   // round j, lane k: pieces first[j][k] .. first[j][k + 1]
    size_t rows_max = 0;
    for (int j = 0; j < rounds; ++j) {
        const long long w0 = (long long)j * C, w1 = w0 + C;
        size_t rows = 0;
        for (int k = 0; k < kXcds; ++k) {
            first[(size_t)j * (kXcds + 1) + k] = (int)pcs.size();
            if (k >= lanes) continue;
            long long u0 = 0;   // lane-time of the utterance's step 0
            for (int u : queue[k]) {
                const long long Lu = (long long)T[u] * hop, a0 = std::max(w0, u0), a1 = std::min(w1, u0 + Lu);
                if (a1 > a0) {
                    const int t0 = (int)(a0 - u0), Lc = (int)(a1 - a0);
                    // the kernels prefetch the terms of the step after the piece while the utterance goes on
                    const int nt = (int)std::min<long long>(Lc + 1, Lu - t0);
                    pcs.push_back({u, t0, Lc, nt});
                    rows += nt;
                }
                u0 += Lu;
            }
        }
        first[(size_t)j * (kXcds + 1) + kXcds] = (int)pcs.size();
        rows_max = std::max(rows_max, rows);
    }

    // ---- every workspace grown before anything is queued (growing one waits for the device)
    const ListArena arena(T, U, nJ, N);
    if (arena.reserve(h) || grow(h, h->d_T, h->T_cap, rows_max * N) ||
        grow(h, h->d_lstate, h->lstate_cap, (size_t)U * kXcdWgs * state_w))
        return WRNN_EHIP;
    HIP_TRY(h, ensure(h->d_lxg, h->lxg_cap, (size_t)U * kXXcdStride));
    HIP_TRY(h, h->ltab.reserve(pcs.size()));
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    if (int rc = blas_on(h, st)) return rc;
    if (int rc = upload_coef(h, coef, st)) return rc;

    // ---- the piece table, all rounds at once: one upload, no host wait between rounds
    for (int j = 0; j < rounds; ++j) {
        size_t row = 0;   // the round's terms rows so far
        int blk = 0;      // … and interpolation blocks
        for (int p = first[(size_t)j * (kXcds + 1)]; p < first[(size_t)j * (kXcds + 1) + kXcds]; ++p) {
            const Piece &pc = pcs[p];
            XcdPiece q{};
            q.r.terms = h->d_T + row * N;
            q.r.terms_ld = N;
            q.r.noise = noise ? noise[pc.u] : nullptr;
            q.r.noise_ld = 11;
            q.r.out = out[pc.u];
            q.r.out_t0 = 0;
            q.r.state = h->d_lstate + (size_t)pc.u * kXcdWgs * state_w;
            q.r.xg = h->d_lxg + (size_t)pc.u * kXXcdStride;
            q.r.seed = seed;
            q.r.row = row_offset + pc.u;
            q.r.t0 = pc.t0;
            q.r.Lc = pc.Lc;
            q.r.L = T[pc.u] * hop;
            q.r.nz_hor = q.r.L;
            q.ft = h->d_larena + arena.ft[pc.u];
            q.at = h->d_larena + arena.at[pc.u];
            q.frames = T[pc.u];
            q.nt = pc.nt;
            q.blk0 = blk;
            h->ltab.h[p] = q;
            row += pc.nt;
            blk += interp_list_blocks(pc.nt);
        }
    }

    // ---- queuing begins
    HIP_TRY(h, h->ltab.upload(pcs.size(), st));
    HIP_TRY(h, hipMemsetAsync(h->d_lxg, 0, (size_t)U * kXXcdStride * 8, st));   // tags restart at 1 in every utterance
    HIP_TRY(h, hipMemsetAsync(h->d_ctl, 0, kCtlWords * sizeof(int), st));
    HIP_TRY(h, hipEventRecord(h->ev0, st));
    set_last_path(h, (int)path);
    const float one = 1.0f, zero = 0.0f;
    const int rc = list_frame_terms(h, mel, aux, T, U, hop, nJ, jlo, arena, N, 0, st, [&](const float *X, int m, float *Cm) -> int {
        if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, m, h->KXc, &one, h->d_xWt,
                          h->KXc, X, h->KXc, &zero, Cm, N) != rocblas_status_success)
            return fail(h, WRNN_EHIP, "rocblas_sgemm (frame terms) failed");
        return WRNN_OK;
    });
    if (rc) return rc;
    for (int j = 0; j < rounds; ++j) {
        const int *f = &first[(size_t)j * (kXcds + 1)];
        int blocks = 0;
        for (int p = f[0]; p < f[kXcds]; ++p) blocks += interp_list_blocks(pcs[p].nt);
        HIP_TRY(h, launch_terms_interp_list(h->ltab.d, f[0], f[kXcds], blocks, h->d_coef, N, hop, nJ, st));
        HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
        auto fill = [&](auto &g, const auto &slab) {
            g.a.slab = h->d_xslab;
            g.a.members = h->d_members;
            g.a.ctl = h->d_ctl;
            g.a.timeout_ticks = h->timeout_ticks;
            g.a.s = slab;
            g.a.windowed = 1;
            g.a.nb = lanes;
            g.pieces = h->ltab.d;
            for (int k = 0; k <= kXcds; ++k) g.first[k] = f[k];
        };
        if (path == P_XCD) {
            XcdListArgs g{};
            fill(g, h->xs);
            HIP_TRY(h, launch_xcd_list(g, st));
        } else {
            XcdsListArgs g{};
            fill(g, h->xss);
            HIP_TRY(h, launch_xcds_list(g, st));
        }
    }
    HIP_TRY(h, hipEventRecord(h->ev1, st));
    h->timed = true;
    return WRNN_OK;
}

// ---- wide lists (wavernn_amd.h: wrnn_list_wide_plan, wrnn_generate_list_wide) ---------------------
// The one-shot use of the grouped launches: up to kMRowsMax slots, each a queue of whole utterances
// (list_plan's assignment).  A slot's timeline is its utterances' steps end to end; all rows of a
// grouped launch run the same number of steps and the kernel takes no per-row mask, so the common
// timeline is cut at every utterance end on any slot, and again wherever a piece between two such
// cuts exceeds the steps budget of its row count.  The rows of a launch are the slots whose timeline
// reaches past its first step, in slot order.
struct WideListPlan {
    std::vector<int> slot_of, pos;
    std::vector<int64_t> slot_frames;
    std::vector<std::vector<int>> queue;   // [slots]: the slots' utterances in running order
    std::vector<WideLaunch> ls;            // off: first timeline step
    long long longest = 0;                 // steps of the longest timeline
};

static int wide_list_plan(const int *T, int U, int slots, int hop, bool raw, WideListPlan &p, std::string *msg) {
    p.slot_of.assign(U, 0);
    p.pos.assign(U, 0);
    p.slot_frames.assign(slots, 0);
    p.queue.assign(slots, {});
    p.ls.clear();
    list_plan(T, U, slots, p.slot_of.data(), p.pos.data(), p.slot_frames.data(), p.queue.data());
    std::vector<long long> cuts, ends(slots);
    p.longest = 0;
    for (int k = 0; k < slots; ++k) {
        long long e = 0;
        for (int u : p.queue[k]) cuts.push_back(e += (long long)T[u] * hop);
        ends[k] = e;
        p.longest = std::max(p.longest, e);
    }
    if (p.longest > INT_MAX) {
        *msg = "the longest slot timeline exceeds the step counter";
        return WRNN_EINVAL;
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    long long prev = 0;
    for (long long c : cuts) {
        int rows = 0;
        for (int k = 0; k < slots; ++k) rows += ends[k] > prev;
        const int Lc_max = wrnn_wide_steps_per_launch(rows, (int)p.longest, raw ? 1 : 0);
        if (Lc_max < 1) {
            *msg = "wrnn_wide_steps_per_launch refused the launch";
            return WRNN_EINVAL;
        }
        push_launches(p.ls, prev, c, Lc_max, rows);
        prev = c;
    }
    return WRNN_OK;
}

static int list_wide_args(const int *frames, int U, int slots, int hop, std::string *msg) {
    if (U < 1) *msg = "a list has at least one utterance";
    else if (slots < 1 || slots > kMRowsMax) *msg = "slots is 1.." + std::to_string(kMRowsMax) + " (16 per XCD)";
    else if (hop < 1) *msg = "hop is at least 1";
    else
        for (int i = 0; i < U; ++i) {
            if (frames[i] < 21)
                *msg = "utterance " + std::to_string(i) + " has " + std::to_string(frames[i]) +
                       " frames: fewer than 21 (the fade-out, as wrnn_postprocess)";
            else if ((long long)frames[i] * hop > INT_MAX)
                *msg = "utterance " + std::to_string(i) + ": hop * frames exceeds the step counter";
            if (!msg->empty()) break;
        }
    return msg->empty() ? WRNN_OK : WRNN_EINVAL;
}

int wrnn_list_wide_plan(const int *frames, int U, int slots, int hop, int raw, int *slot_of, int *pos_in_slot,
                        int64_t *slot_frames, int *launch_first, int *launch_steps, int *launch_rows, int cap) {
    if (!frames) return cond_fail(WRNN_EINVAL, "need frames");
    std::string msg;
    if (int rc = list_wide_args(frames, U, slots, hop, &msg)) return cond_fail(rc, msg);
    WideListPlan p;
    if (int rc = wide_list_plan(frames, U, slots, hop, raw != 0, p, &msg)) return cond_fail(rc, msg);
    for (int i = 0; i < U; ++i) {
        if (slot_of) slot_of[i] = p.slot_of[i];
        if (pos_in_slot) pos_in_slot[i] = p.pos[i];
    }
    for (int k = 0; k < slots; ++k)
        if (slot_frames) slot_frames[k] = p.slot_frames[k];
    return emit_launches(p.ls, launch_first, launch_steps, launch_rows, cap);
}

// The checks a wide list and a folded list share, before anything is queued or any workspace touched:
// the handle has the grouped many-row form, the upsample config matches it and has an exact
// frame-rate form → hop, nJ, jlo and the frame weights.
static int wide_list_handle_args(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *aux, int *hop_out,
                                 int *nJ_out, int *jlo_out, std::vector<float> &coef) {
    if (h->dm)
        return fail(h, WRNN_EUNSUPPORTED, "wide lists run the many-row XCD kernel (MoL, or RAW with 9 bits; rnn / fc 512): "
                                          "this handle is a deepmind one");
    const std::string why = wide_refusal(h);
    if (!why.empty()) return fail(h, WRNN_EUNSUPPORTED, why);
    return list_upsample(h, ucfg, aux, hop_out, nJ_out, jlo_out, coef);
}

// What a wide list and a folded list share from the first check to the reserved row table.  Their
// difference is two callables, each (front, &msg) → a WRNN_ code, that refuse what is theirs to
// refuse — `before_ptrs` ahead of the per-utterance pointer check, `after_ptrs` behind it — and between
// them leave the launches in `ls` and the number of state records in `n_state`.
struct WideListFront {
    int hop = 1, nJ = 1, jlo = 0, K = 11;
    bool raw = false;
    hipStream_t st = nullptr;
    std::vector<WideLaunch> ls;          // the launches of the call (filled by the entry point's callables)
    int n_state = 0;                     // state records: one per utterance (wide) or per fold (folded)
    size_t ntab = 0;                     // row records of all launches
    ListArena arena;
};

template <typename Before, typename After>
static int wide_list_front(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                           const int *T, int U, const float *const *noise, float *const *out, void *stream,
                           Before before_ptrs, After after_ptrs, bool folds, WideListFront &f) {
    if (!h) return WRNN_EINVAL;
    if (!h->ready) return fail(h, WRNN_ENOWEIGHTS, "weights not (fully) set");
    // ---- every argument of every utterance, before anything is queued or any workspace touched
    if (!ucfg || !mel || !T || !out || U < 1) return fail(h, WRNN_EINVAL, "need ucfg, mel, T, out and U >= 1");
    std::vector<float> coef;
    if (int rc = wide_list_handle_args(h, ucfg, aux, &f.hop, &f.nJ, &f.jlo, coef)) return rc;
    f.raw = h->cfg.mode == WRNN_MODE_RAW;
    f.K = f.raw ? kMRawNC : 11;
    const int A4 = h->CD - h->cfg.feat_dims;
    std::string msg;
    if (int rc = before_ptrs(f, &msg)) return fail(h, rc, msg);
    for (int i = 0; i < U; ++i)
        if (!mel[i] || !out[i] || (A4 > 0 && !aux[i]) || (noise && !noise[i]))
            return fail(h, WRNN_EINVAL, "utterance " + std::to_string(i) + ": need mel, aux, out (and its noise)");
    if (int rc = after_ptrs(f, &msg)) return fail(h, rc, msg);
    HIP_TRY(h, hipSetDevice(h->device));
    f.st = (hipStream_t)stream;

    // ---- every workspace grown before anything is queued (growing one waits for the device)
    const int N = kXcdWgs * kMRing;
    f.arena = ListArena(T, U, f.nJ, N);
    size_t t_need = 0, nz_need = 0;
    for (const WideLaunch &l : f.ls) {
        f.ntab += (size_t)l.rows;
        t_need = std::max(t_need, (size_t)(l.Lc + 1) * l.rows * N);   // one row on: the kernel's look-ahead load
        nz_need = std::max(nz_need, (size_t)(l.Lc + 1) * l.rows * f.K);
    }
    if (f.arena.reserve(h) || grow(h, h->d_T, h->T_cap, t_need) || grow(h, h->d_xmnoise, h->xmnoise_cap, nz_need) ||
        grow(h, h->d_lstate, h->lstate_cap, (size_t)f.n_state * kXcdWgs * kMRowStateW))
        return WRNN_EHIP;
    // the hop area, rocBLAS on the stream and the frame weights on the device
    if (!h->d_xmxg) HIP_TRY(h, hipMalloc(&h->d_xmxg, (size_t)kXcds * kMXcdStride * 8));
    if (int rc = blas_on(h, f.st)) return rc;
    if (int rc = upload_coef(h, coef, f.st)) return rc;
    return wide_tab_reserve(h, f.ntab + (folds ? fold_tab_records(f.ntab) : 0));
}

// Each utterance's frame-term stores in the list arena, with the launches and shapes of its own
// wrnn_generate_frames call on the many-row path (never one GEMM over several utterances)
static int wide_list_frame_terms(wrnn_t *h, const float *const *mel, const float *const *aux, const int *T, int U,
                                 const WideListFront &f) {
    const int N = kXcdWgs * kMRing;
    const float one = 1.0f, zero = 0.0f;
    XcdmGemm gemms[3];
    xcdm_terms_gemms(*h, gemms);
    return list_frame_terms(h, mel, aux, T, U, f.hop, f.nJ, f.jlo, f.arena, N, h->cfg.feat_dims + h->cfg.aux_dims, f.st,
                            [&](const float *X, int m, float *C) -> int {
        for (const XcdmGemm &g : gemms)
            if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, g.rows, m, g.k, &one,
                              h->d_xmWt + (size_t)g.row0 * h->KXc + g.col0, h->KXc, X + g.col0, h->KXc, &zero, C + g.row0,
                              N) != rocblas_status_success)
                return fail(h, WRNN_EHIP, "rocblas_sgemm (frame terms) failed");
        return WRNN_OK;
    });
}

int wrnn_generate_list_wide(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                            const int *T, int U, int slots, const float *const *noise, uint64_t seed, int64_t row_offset,
                            float *const *out, void *stream) {
    if (slots == 0) slots = std::min(kMRowsMax, U);
    WideListPlan p;
    WideListFront f;
    if (int rc = wide_list_front(
            h, ucfg, mel, aux, T, U, noise, out, stream,
            [&](WideListFront &w, std::string *msg) { return list_wide_args(T, U, slots, w.hop, msg); },
            [&](WideListFront &w, std::string *msg) {
                const int rc = wide_list_plan(T, U, slots, w.hop, w.raw, p, msg);
                w.ls = p.ls;
                w.n_state = U;
                return rc;
            },
            false, f))
        return rc;
    const int N = kXcdWgs * kMRing, hop = f.hop, K = f.K;
    const size_t ntab = f.ntab;

    // ---- the row tables of all launches: a launch lies inside one utterance of every slot it runs,
    // found by walking each slot's queue along the timeline (cur: the slot's utterance, u0: its first step)
    std::vector<int> cur(slots, 0);
    std::vector<long long> u0(slots, 0);
    size_t at = 0;
    for (const WideLaunch &l : f.ls) {
        for (int k = 0; k < slots; ++k) {
            const std::vector<int> &q = p.queue[k];
            while (cur[k] < (int)q.size() && u0[k] + (long long)T[q[cur[k]]] * hop <= l.off)
                u0[k] += (long long)T[q[cur[k]++]] * hop;
            if (cur[k] >= (int)q.size()) continue;   // the slot's queue has ended: it takes no row
            const int i = q[cur[k]], t0 = (int)(l.off - u0[k]);
            if (t0 < 0 || (long long)t0 + l.Lc > (long long)T[i] * hop)
                return fail(h, WRNN_EINVAL, "wide list: a launch leaves its utterance");
            XcdmRow r{};
            r.ft = h->d_larena + f.arena.ft[i];
            r.at = h->d_larena + f.arena.at[i];
            r.fr_ld = N;
            r.noise = noise ? noise[i] + (size_t)t0 * K : nullptr;
            r.noise_ld = K;
            r.seed = seed;
            r.prow = row_offset + i;
            r.out = out[i] + t0;
            r.state = h->d_lstate + (size_t)i * kXcdWgs * kMRowStateW;   // the utterance's own record
            r.ft_base = r.at_base = 0;
            r.t0 = t0;
            r.resume = t0 > 0;
            if (at >= ntab) return fail(h, WRNN_EINVAL, "wide list: the row tables do not match the plan");
            h->wtab.h[at++] = r;
        }
    }
    if (at != ntab) return fail(h, WRNN_EINVAL, "wide list: the row tables do not match the plan");

    // ---- queuing begins
    if (int rc = wide_list_frame_terms(h, mel, aux, T, U, f)) return rc;
    return wide_run_launches(h, f.ls, ntab, h->d_coef, hop, f.nJ, f.raw, K, f.st);
}

// ---- folded lists (wavernn_amd.h: wrnn_list_folds_plan, wrnn_generate_list_folds) ------------------
// The folds of all utterances, numbered utterance-major, are the rows: fold g runs in round g / slots
// as launch row g % slots.  Folds are all Lf = target + 2·overlap steps, so the common timeline is cut
// at round ends only, and again wherever a round exceeds the steps budget of its row count.
struct FoldListPlan {
    std::vector<int> folds, first_row;
    int F = 0, slots = 0, Lf = 0;
    std::vector<WideLaunch> ls;   // off: first fold-local step (the launches of round q follow those of round q − 1)
    std::vector<int> round_of;    // [launches]
};

static int fold_list_plan(const int *frames, int U, int hop, int target, int overlap, int slots, bool raw, FoldListPlan &p,
                          std::string *msg) {
    if (U < 1) *msg = "a list has at least one utterance";
    else if (slots < 0 || slots > kMRowsMax) *msg = "slots is 1.." + std::to_string(kMRowsMax) + " (16 per XCD), or 0 for min(" + std::to_string(kMRowsMax) + ", folds)";
    else if (hop < 1) *msg = "hop is at least 1";
    else if (target < 1) *msg = "target is at least 1";
    else if (overlap < 0) *msg = "overlap is at least 0";
    else if ((long long)target + 2LL * overlap > INT_MAX) *msg = "target + 2 * overlap exceeds the step counter";
    if (!msg->empty()) return WRNN_EINVAL;
    p.folds.assign(U, 0);
    p.first_row.assign(U, 0);
    p.ls.clear();
    p.round_of.clear();
    p.Lf = target + 2 * overlap;
    const long long stride = (long long)target + overlap;
    long long F = 0;
    for (int i = 0; i < U; ++i) {
        const std::string who = "utterance " + std::to_string(i);
        const long long L = (long long)frames[i] * hop;
        if (frames[i] < 21)
            *msg = who + " has " + std::to_string(frames[i]) + " frames: fewer than 21 (the fade-out, as wrnn_postprocess)";
        else if (L > (1LL << 30)) *msg = who + ": hop * frames exceeds the step counter";
        else if (L < overlap) *msg = who + ": hop * frames (" + std::to_string(L) + ") is less than the overlap";
        if (!msg->empty()) return WRNN_EINVAL;
        // fold_with_overlap's count (condition.hip: fold_geometry, what wrnn_cond_shape returns)
        long long n = (L - overlap) / stride;
        if (L - (n * stride + overlap) != 0) ++n;
        if (n < 1) *msg = who + ": hop * frames equals the overlap: no fold";
        else if ((n - 1) * stride + p.Lf > INT_MAX) *msg = who + ": its folds exceed the step counter";
        else if (F + n > INT_MAX) *msg = "the list has more folds than the row counter holds";
        if (!msg->empty()) return WRNN_EINVAL;
        p.folds[i] = (int)n;
        p.first_row[i] = (int)F;
        F += n;
    }
    p.F = (int)F;
    p.slots = slots == 0 ? (int)std::min<long long>(kMRowsMax, F) : slots;
    const long long rounds = (F + p.slots - 1) / p.slots;
    if (rounds * p.Lf > INT_MAX) {
        *msg = "the common timeline (rounds * (target + 2 * overlap)) exceeds the step counter";
        return WRNN_EINVAL;
    }
    for (long long q = 0; q < rounds; ++q) {
        const int rows = (int)std::min<long long>(p.slots, F - q * p.slots);
        const int Lc_max = wrnn_wide_steps_per_launch(rows, p.Lf, raw ? 1 : 0);
        if (Lc_max < 1) {
            *msg = "wrnn_wide_steps_per_launch refused the launch";
            return WRNN_EINVAL;
        }
        push_launches(p.ls, 0, p.Lf, Lc_max, rows);
        p.round_of.resize(p.ls.size(), (int)q);
    }
    return WRNN_OK;
}

int wrnn_list_folds_plan(const int *frames, int U, int hop, int target, int overlap, int slots, int raw, int *folds,
                         int *first_row, int *launch_first, int *launch_steps, int *launch_rows, int cap) {
    if (!frames) return cond_fail(WRNN_EINVAL, "need frames");
    std::string msg;
    FoldListPlan p;
    if (int rc = fold_list_plan(frames, U, hop, target, overlap, slots, raw != 0, p, &msg)) return cond_fail(rc, msg);
    for (int i = 0; i < U; ++i) {
        if (folds) folds[i] = p.folds[i];
        if (first_row) first_row[i] = p.first_row[i];
    }
    for (size_t j = 0; launch_first && j < p.ls.size() && (int)j < cap; ++j)
        launch_first[j] = p.round_of[j] * p.Lf + p.ls[j].off;   // on the common timeline, not fold-local
    return emit_launches(p.ls, nullptr, launch_steps, launch_rows, cap);
}

int wrnn_generate_list_folds(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                             const int *T, int U, int target, int overlap, int slots, const float *const *noise,
                             uint64_t seed, int64_t row_offset, float *const *out, void *stream) {
    FoldListPlan p;
    WideListFront fr;
    if (int rc = wide_list_front(
            h, ucfg, mel, aux, T, U, noise, out, stream,
            [&](WideListFront &w, std::string *msg) {   // the fold plan refuses everything before the pointers
                const int rc = fold_list_plan(T, U, w.hop, target, overlap, slots, w.raw, p, msg);
                w.ls = p.ls;
                w.n_state = p.F;
                return rc;
            },
            [](WideListFront &, std::string *) { return (int)WRNN_OK; }, true, fr))
        return rc;
    const int N = kXcdWgs * kMRing, K = fr.K;
    const size_t ntab = fr.ntab;

    // ---- the row tables of all launches, the fold records behind them in the same order
    FoldRow *h_folds = reinterpret_cast<FoldRow *>(h->wtab.h + ntab);
    const int stride = target + overlap;
    size_t at = 0;
    for (size_t j = 0; j < p.ls.size(); ++j) {
        const WideLaunch &l = p.ls[j];
        int i = 0;   // the utterance of the round's first fold, then onwards: folds are utterance-major
        const int g0 = p.round_of[j] * p.slots;
        while (i + 1 < U && p.first_row[i + 1] <= g0) ++i;
        for (int r = 0; r < l.rows; ++r) {
            const int g = g0 + r;
            while (g >= p.first_row[i] + p.folds[i]) ++i;
            const int f = g - p.first_row[i], nf = p.folds[i];
            if (at >= ntab || i >= U || f < 0) return fail(h, WRNN_EINVAL, "folded list: the row tables do not match the plan");
            XcdmRow row{};
            row.ft = h->d_larena + fr.arena.ft[i];
            row.at = h->d_larena + fr.arena.at[i];
            row.fr_ld = N;
            row.noise = noise ? noise[i] + ((size_t)l.off * nf + f) * K : nullptr;   // [Lf][folds_i][K]
            row.noise_ld = (long long)nf * K;
            row.seed = seed;
            row.prow = row_offset + g;
            row.out = out[i] + (size_t)f * p.Lf + l.off;                             // [folds_i][Lf]
            row.state = h->d_lstate + (size_t)g * kXcdWgs * kMRowStateW;             // the fold's own record
            row.ft_base = row.at_base = 0;
            row.t0 = l.off;                                                          // the fold-local step (Philox)
            row.resume = l.off > 0;
            h_folds[at] = FoldRow{f * stride + l.off, T[i]};
            h->wtab.h[at++] = row;
        }
    }
    if (at != ntab) return fail(h, WRNN_EINVAL, "folded list: the row tables do not match the plan");

    // ---- queuing begins
    if (int rc = wide_list_frame_terms(h, mel, aux, T, U, fr)) return rc;
    return wide_run_launches(h, fr.ls, ntab, h->d_coef, fr.hop, fr.nJ, fr.raw, K, fr.st, true);
}
