// capi_stream.cpp — streaming sessions of the C-ABI host: open / push / close, narrow groups on the
// one-row XCD kernels, wide groups on the many-row kernel (whose launch loop the wide lists share),
// rows sessions on the multi-row kernel (any fatchord model; generate_rows' launch loop).
#include "host_ctx.h"

using namespace wrnn;
using namespace wrnn::host;

// ---- streaming sessions (wavernn_amd.h: wrnn_stream_*) ------------------------------------
// Rows [base, end) of `row` floats each in absolute numbering, appended at `end`; rows behind
// keep_from may go.  When the live buffer is full the kept rows move to the front of the other one
// (so the copy never overlaps), which is then the live one: old rows are copied, never recomputed.
struct RowWin {
    float *buf[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};   // floats
    int cur = 0;
    long long base = 0, end = 0;
    size_t row = 0;
    float *at(long long r) { return buf[cur] + (size_t)(r - base) * row; }
};

static int win_reserve(wrnn_t *h, RowWin &w, long long keep_from, long long add, hipStream_t st) {
    keep_from = std::min(std::max(keep_from, w.base), w.end);
    if ((size_t)(w.end + add - w.base) * w.row <= w.cap[w.cur]) return WRNN_OK;
    const int o = 1 - w.cur;
    const size_t need = (size_t)(w.end - keep_from + add) * w.row;
    // ensure() frees through hipFree, which waits for the device: no launch in flight reads buf[o]
    if (need > w.cap[o]) HIP_TRY(h, ensure(w.buf[o], w.cap[o], 2 * need));
    if (w.end > keep_from)
        HIP_TRY(h, hipMemcpyAsync(w.buf[o], w.at(keep_from), (size_t)(w.end - keep_from) * w.row * sizeof(float),
                                  hipMemcpyDeviceToDevice, st));
    w.cur = o;
    w.base = keep_from;
    return WRNN_OK;
}

struct wrnn_stream {
    wrnn_t *h = nullptr;
    int device = 0;
    LoopPath path = P_XCD;
    bool wide = false;              // wrnn_stream_open_wide: the many-row kernel's grouped launches (path P_XCDM)
    bool raw = false;               // a RAW handle's session (wide only): the softmax head, noise_k = kMRawNC Exp(1) draws
    bool mu_law = false;            // RAW: wrnn_stream_mu_law — the emitted samples are mu-law expanded
    bool rows = false;              // wrnn_stream_open_rows: the multi-row kernel over per-sample records (path P_ROWS)
    int noise_k = 11;               // draws per row-step
    int U = 0, T_known = -1;
    wrnn_upsample_cfg ucfg{};
    std::vector<float> taps[4];
    wrnn_melresnet_cfg mcfg{};
    const float *mr_packed = nullptr, *noise = nullptr;
    int noise_steps = 0;
    uint64_t seed = 0;
    int64_t row_offset = 0;
    int hop = 1, nJ = 1, jlo = 0, pad = 0;
    int N = 0, state_w = 0;
    // progress: frames received, aux frames formed, loop steps run, samples emitted
    int R = 0, A = 0, steps = 0, audio = 0;
    bool fin = false, dead = false, primed = false;
    unsigned long long loads = 0;   // the handle's load count at wrnn_stream_open
    // device state of the session
    float *d_coef = nullptr, *d_state = nullptr, *d_tail[2] = {nullptr, nullptr};
    unsigned long long *d_xg = nullptr;
    int tail_cur = 0;
    RowWin FT, AT;                  // W·(mel frame) rows i = frame − jlo, W·(aux frame, ones) rows f
    float *d_y[2] = {nullptr, nullptr};   // fp32 loop samples not yet emitted: [U][y_ld], column 0 = step y_t0
    size_t y_cap[2] = {0, 0};
    int y_ld[2] = {0, 0}, y_cur = 0, y_t0 = 0;
    // per-push workspaces
    float *d_win = nullptr, *d_aux = nullptr, *d_frec = nullptr, *d_X = nullptr, *d_T = nullptr;
    size_t win_cap = 0, aux_cap = 0, frec_cap = 0, X_cap = 0, T_cap = 0;
    // rows sessions: frames kept behind the newest mel / aux frame (the records of the next steps read
    // them), the aux tail [keep][U][A4], the windows and records of a push, the layout of d_state
    int mel_keep = 0, aux_keep = 0, atail_cur = 0, rows_ng = 0;
    size_t rows_state_grp = 0;
    float *d_atail[2] = {nullptr, nullptr}, *d_mwin = nullptr, *d_awin = nullptr, *d_cond = nullptr;
    size_t mwin_cap = 0, awin_cap = 0, cond_cap = 0;
};

static int hop_of(const wrnn_upsample_cfg *c, int *hop) {
    if (!c || c->n_scales < 1 || c->n_scales > 4 || c->pad < 0) return WRNN_EINVAL;
    long long hh = 1;
    for (int i = 0; i < c->n_scales; ++i) {
        if (c->scales[i] < 1) return WRNN_EINVAL;
        hh *= c->scales[i];
    }
    if (hh > (1 << 20)) return WRNN_EINVAL;
    *hop = (int)hh;
    return WRNN_OK;
}

// The emission rule of wavernn_amd.h: counts after R frames.  msg: why it is WRNN_EINVAL.
static int stream_counts(int hop, int look, long long R, bool final, long long T_known, long long *steps,
                         long long *audio, std::string *msg) {
    const long long kFadeFrames = 20;   // generate()'s fade-out: 20·hop_length samples (fatchord_version.py:255-258)
    if (R < 0 || T_known < -1) {
        *msg = "negative frame count";
        return WRNN_EINVAL;
    }
    const long long T = final ? R : T_known;
    if (final && T_known >= 0 && R != T_known) {
        *msg = "final after " + std::to_string(R) + " frames, total_frames was " + std::to_string(T_known);
        return WRNN_EINVAL;
    }
    if (!final && T_known >= 0 && R > T_known) {
        *msg = std::to_string(R) + " frames pushed, total_frames was " + std::to_string(T_known);
        return WRNN_EINVAL;
    }
    if (T >= 0 && T < kFadeFrames + 1) {
        *msg = "operands could not be broadcast together: the fade-out (20*hop_length = " +
               std::to_string(kFadeFrames * hop) + ") is longer than the waveform (" +
               std::to_string(std::max(0LL, T - 1) * hop) + ")";
        return WRNN_EINVAL;
    }
    if ((std::max(R, T) + 1) * hop > (1LL << 31) - 1) {
        *msg = "step index past 2^31";
        return WRNN_EINVAL;
    }
    if (final) {
        *steps = T * hop;
        *audio = (T - 1) * hop;
    } else {
        *steps = std::max(0LL, R - look) * hop;
        *audio = std::min(*steps, T >= 0 ? (T - 1) * hop : std::max(0LL, (R - (kFadeFrames + 1)) * hop));
    }
    return WRNN_OK;
}

int wrnn_stream_lookahead(const wrnn_upsample_cfg *ucfg) {
    int hop = 1;
    if (int rc = hop_of(ucfg, &hop)) return cond_fail(rc, "bad upsample config");
    return ucfg->pad + 1;
}

int wrnn_stream_plan(const wrnn_upsample_cfg *ucfg, int frames_received, int final, int total_frames,
                     int64_t *steps_done, int64_t *audio_done) {
    int hop = 1;
    if (int rc = hop_of(ucfg, &hop)) return cond_fail(rc, "bad upsample config");
    long long s = 0, a = 0;
    std::string msg;
    if (int rc = stream_counts(hop, ucfg->pad + 1, frames_received, final != 0, total_frames, &s, &a, &msg))
        return cond_fail(rc, msg);
    if (steps_done) *steps_done = s;
    if (audio_done) *audio_done = a;
    return WRNN_OK;
}

void wrnn_stream_close(wrnn_stream_t *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void *p : {(void *)s->d_coef, (void *)s->d_state, (void *)s->d_tail[0],
                    (void *)s->d_tail[1], (void *)s->d_xg, (void *)s->FT.buf[0], (void *)s->FT.buf[1],
                    (void *)s->AT.buf[0], (void *)s->AT.buf[1], (void *)s->d_y[0], (void *)s->d_y[1], (void *)s->d_win,
                    (void *)s->d_aux, (void *)s->d_frec, (void *)s->d_X, (void *)s->d_T, (void *)s->d_atail[0],
                    (void *)s->d_atail[1], (void *)s->d_mwin, (void *)s->d_awin, (void *)s->d_cond})
        if (p) (void)hipFree(p);   // hipFree waits for the device: no push in flight uses them
    delete s;
}

// Why a MoL or RAW handle has no grouped many-row form (wrnn_stream_open_wide and
// wrnn_generate_list_wide refuse it with WRNN_EUNSUPPORTED and this text), or "" when it has one
std::string wrnn::host::wide_refusal(const wrnn_t *h) {
    if (h->cfg.mode == WRNN_MODE_RAW) {   // the many-row kernel's softmax head: which of its conditions this handle misses
        if (h->cfg.n_classes != kMRawNC)
            return "wide RAW streaming sessions run the many-row XCD kernel's softmax head of " + std::to_string(kMRawNC) +
                   " classes (bits = 9): this handle has " + std::to_string(h->cfg.n_classes) + " classes";
        if (h->cfg.rnn_dims != 512 || h->cfg.fc_dims != 512)
            return "wide RAW streaming sessions run the many-row XCD kernel (rnn / fc 512): this handle has rnn " +
                   std::to_string(h->cfg.rnn_dims) + ", fc " + std::to_string(h->cfg.fc_dims);
        if (!(h->xcdm_ok && h->xcdm_nq >= kMQuadMax))
            return "wide RAW streaming sessions run the many-row XCD kernel with four co-resident quads per XCD (aux 32, a "
                   "full MI355X): this handle does not have the four-quad form";
        if (!h->xcdmg_ok)
            return "wide RAW streaming sessions run the many-row XCD kernel's grouped RAW instantiation: it is not "
                   "co-resident on this device";
    }
    if (!(h->xcdm_ok && h->xcdmg_ok && h->xcdm_nq >= kMQuadMax))
        return "wide streaming sessions run the many-row XCD kernel with four co-resident quads per XCD (MoL, rnn / fc "
               "512, a full MI355X): this handle does not have it";
    return std::string();
}

// ---- rows sessions (wrnn_stream_open_rows): set-up ----------------------------------------------
// The block generate_rows would run for the session's U rows, with the partition it picks swapped in
// for the call only.  WRNN_OK with k->Bl < U when U rows are more than one row block.
static int rows_session_block(wrnn_t *h, int U, int steps, RowsBlock *k) {
    const bool grouped = rows_grouped(*h, U);
    PartScope ps(*h, h->g2, grouped);
    return rows_block(h, grouped, U, steps, k);
}

// Largest row count generate_rows runs as ONE row block for this handle (its rows_tile_for loop,
// capped at kRowsMax): the tile fit only loosens with fewer rows, so the first fit from above is it
static int rows_one_block_max(wrnn_t *h) {
    for (int U = kRowsMax; U > 1; --U) {
        RowsBlock k;
        if (rows_session_block(h, U, 1, &k) == WRNN_OK && k.Bl == U) return U;
    }
    return 1;
}

// The frames the records of a step reach, behind and ahead, from wrnn_upsample_window_frames at a step
// far from either end (the reach does not depend on the frame, only on the phase: a frame's first
// step reaches furthest back, its last furthest ahead).  Ahead they must stay inside the look-ahead:
// after R frames the session runs steps below (R − pad − 1)·hop, and those may read no frame >= R.
static int rows_reach(wrnn_stream *s) {
    wrnn_t *h = s->h;
    const int q = 64, pad = s->pad, hop = s->hop;
    int lo = 0, hi = 0, alo = 0, ahi = 0;
    if (int rc = wrnn_upsample_window_frames(&s->ucfg, -1, q * hop, hop, &lo, &hi, &alo, &ahi))
        return fail(h, rc, std::string("upsample window: ") + wrnn_cond_last_error());
    if (hi > q + pad + 2)   // frame q's steps run once R = q + pad + 2 frames are in: frames [.., R)
        return fail(h, WRNN_EUNSUPPORTED, "the upsample cascade reads " + std::to_string(hi - q - 1) + " frames ahead of a "
                                          "step's own: more than the look-ahead of " + std::to_string(pad + 1));
    // the oldest step of a push is (R_old − pad − 1)·hop: its frame, pad + 1 behind the newest, and the reach behind it
    s->mel_keep = std::max(2 * pad, pad + 1 + std::max(0, q - lo));
    s->aux_keep = 1;   // aux frames exist up to R − pad, the oldest step's own is R − pad − 1
    return WRNN_OK;
}

static int rows_open_buffers(wrnn_stream *s) {
    wrnn_t *h = s->h;
    const int U = s->U, feat = h->cfg.feat_dims, A4 = h->CD - feat;
    RowsBlock k;
    if (int rc = rows_session_block(h, U, 1, &k)) return rc;
    s->rows_ng = k.ng;
    s->rows_state_grp = k.state_grp;
    const size_t state_n = (size_t)k.ng * k.state_grp;
    const size_t mt = (size_t)std::max(1, s->mel_keep) * U * feat, at = (size_t)s->aux_keep * U * std::max(1, A4);
    HIP_TRY(h, hipMalloc(&s->d_state, state_n * sizeof(float)));
    HIP_TRY(h, hipMemset(s->d_state, 0, state_n * sizeof(float)));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(h, hipMalloc(&s->d_tail[i], mt * sizeof(float)));
        HIP_TRY(h, hipMemset(s->d_tail[i], 0, mt * sizeof(float)));
        HIP_TRY(h, hipMalloc(&s->d_atail[i], at * sizeof(float)));
        HIP_TRY(h, hipMemset(s->d_atail[i], 0, at * sizeof(float)));
    }
    HIP_TRY(h, hipDeviceSynchronize());   // the memsets are asynchronous to the host
    return WRNN_OK;
}

static int stream_open(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                       const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                       uint64_t seed, int64_t row_offset, wrnn_stream_t **out, bool wide, bool rows = false) {
    if (!h) return WRNN_EINVAL;
    if (!out) return fail(h, WRNN_EINVAL, "need out");
    *out = nullptr;
    if (!h->ready) return fail(h, WRNN_ENOWEIGHTS, "weights not (fully) set");
    if (!ucfg || !mcfg || !melresnet_packed) return fail(h, WRNN_EINVAL, "need ucfg, mcfg and the packed MelResNet");
    if (rows) {   // any fatchord handle the multi-row kernel runs, as many rows as one row block of it holds
        if (h->dm)
            return fail(h, WRNN_EUNSUPPORTED, "rows sessions run the fatchord multi-row kernel: this handle is a deepmind "
                                              "one (it takes no conditioning)");
        if (!h->rows_ok)
            return fail(h, WRNN_EUNSUPPORTED, "rows sessions run the multi-row kernel: this handle does not have it (its "
                                              "weights fit neither LDS nor the streamed form on this device)");
        const int lim = rows_one_block_max(h);
        if (U < 1 || U > lim)
            return fail(h, WRNN_EINVAL, "a rows session has 1.." + std::to_string(lim) + " utterances (one row block of the "
                                        "multi-row kernel for this handle), not " + std::to_string(U));
    }
    const int U_max = rows ? kRowsMax : wide ? kMRowsMax : kXcds;
    if (U < 1 || U > U_max) return fail(h, WRNN_EINVAL, std::string(wide ? "a wide session" : "a session") + " has 1.." +
                                                            std::to_string(U_max) + " utterances");
    if (total_frames < -1) return fail(h, WRNN_EINVAL, "total_frames is a frame count or -1");
    if (noise && noise_steps < 1) return fail(h, WRNN_EINVAL, "noise needs noise_steps >= 1");
    const bool raw = !h->dm && h->cfg.mode == WRNN_MODE_RAW;
    if (h->dm || (h->cfg.mode != WRNN_MODE_MOL && !(raw && (wide || rows))))
        return fail(h, WRNN_EUNSUPPORTED, "streaming sessions run the one-row XCD MoL kernels: this handle is not MoL");
    if (wide) {
        const std::string why = wide_refusal(h);
        if (!why.empty()) return fail(h, WRNN_EUNSUPPORTED, why);
    }
    const LoopPath path = rows ? P_ROWS : wide ? P_XCDM : choose_path(h, U);
    if (!wide && !rows && path != P_XCD && path != P_XCDS)
        return fail(h, WRNN_EUNSUPPORTED,
                    "streaming sessions run the dense rnn/fc 512 XCD kernel or the block-sparse rnn 896 one; " +
                        std::to_string(U) + " row(s) of this handle take loop path " + std::to_string((int)path));
    const int feat = h->cfg.feat_dims, A4 = h->CD - feat;
    if (ucfg->feat_dims != feat || ucfg->res_out_dims != A4 || mcfg->in_dims != feat || mcfg->res_out_dims != A4 ||
        mcfg->pad != ucfg->pad)
        return fail(h, WRNN_EINVAL, "upsample / MelResNet config does not match the handle's feat / aux dims");
    if (int rc = check_upsample_scales(h, ucfg)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    std::unique_ptr<wrnn_stream, void (*)(wrnn_stream *)> s(new wrnn_stream, wrnn_stream_close);
    s->h = h;
    s->device = h->device;
    s->loads = h->loads;
    s->path = path;
    s->wide = wide;
    s->rows = rows;
    s->raw = raw;
    s->noise_k = rows ? h->NK : raw ? kMRawNC : 11;
    s->U = U;
    s->T_known = total_frames;
    s->ucfg = *ucfg;
    for (int i = 0; i < ucfg->n_scales; ++i) {
        s->taps[i].assign(ucfg->taps[i], ucfg->taps[i] + 2 * ucfg->scales[i] + 1);
        s->ucfg.taps[i] = s->taps[i].data();
    }
    s->mcfg = *mcfg;
    s->mr_packed = melresnet_packed;
    s->noise = noise;
    s->noise_steps = noise_steps;
    s->seed = seed;
    s->row_offset = row_offset;
    s->pad = ucfg->pad;
    std::vector<float> coef;
    if (rows) {   // per-sample records: the cascade needs no frame-rate form, only to stay inside the look-ahead
        if (hop_of(&s->ucfg, &s->hop)) return fail(h, WRNN_EINVAL, "bad upsample config");
        if (int rc = rows_reach(s.get())) return rc;
    } else if (int rc = frame_form(h, &s->ucfg, &s->hop, &s->nJ, &s->jlo, coef)) {
        return rc;
    }
    if (total_frames >= 0) {   // the same refusal final would give, before any work
        long long st_ = 0, au_ = 0;
        std::string msg;
        if (int rc = stream_counts(s->hop, s->pad + 1, 0, false, total_frames, &st_, &au_, &msg)) return fail(h, rc, msg);
    }
    const int tile = wrnn_melresnet_tile_frames(mcfg, U, 1);
    if (tile < 0) return fail(h, tile, "the MelResNet kernel does not cover these channel counts");
    if (rows) {
        if (int rc = rows_open_buffers(s.get())) return rc;
        *out = s.release();
        return WRNN_OK;
    }
    // wide: the many-row kernel's compact record and one state record per row and workgroup; its
    // launches restart their tags over the handle's hop area, so the session owns no granules
    s->N = kXcdWgs * (wide ? kMRing : path == P_XCD ? kXTerms : kSTerms);
    s->state_w = wide ? kMRowStateW : path == P_XCD ? kXStateW : kSStateW;
    s->FT.row = s->AT.row = (size_t)U * s->N;
    const size_t tail_n = (size_t)std::max(1, 2 * s->pad) * U * feat;
    HIP_TRY(h, hipMalloc(&s->d_coef, coef.size() * sizeof(float)));
    HIP_TRY(h, hipMalloc(&s->d_state, (size_t)U * kXcdWgs * s->state_w * sizeof(float)));
    if (wide) {
        if (!h->d_xmxg) HIP_TRY(h, hipMalloc(&h->d_xmxg, (size_t)kXcds * kMXcdStride * 8));
    } else {
        HIP_TRY(h, hipMalloc(&s->d_xg, (size_t)U * kXXcdStride * 8));
    }
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(h, hipMalloc(&s->d_tail[i], tail_n * sizeof(float)));
        HIP_TRY(h, hipMemset(s->d_tail[i], 0, tail_n * sizeof(float)));
    }
    HIP_TRY(h, hipMemcpy(s->d_coef, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice));
    if (s->d_xg) HIP_TRY(h, hipMemset(s->d_xg, 0, (size_t)U * kXXcdStride * 8));   // hop tags are step + 1: they start at 1
    HIP_TRY(h, hipMemset(s->d_state, 0, (size_t)U * kXcdWgs * s->state_w * sizeof(float)));
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    HIP_TRY(h, hipDeviceSynchronize());   // the memsets are asynchronous to the host
    *out = s.release();
    return WRNN_OK;
}

int wrnn_stream_open(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                     const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                     uint64_t seed, int64_t row_offset, wrnn_stream_t **out) {
    return stream_open(h, ucfg, mcfg, melresnet_packed, U, total_frames, noise, noise_steps, seed, row_offset, out, false);
}

int wrnn_stream_open_rows(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                          const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                          uint64_t seed, int64_t row_offset, wrnn_stream_t **out) {
    return stream_open(h, ucfg, mcfg, melresnet_packed, U, total_frames, noise, noise_steps, seed, row_offset, out, false,
                       true);
}

int wrnn_stream_mu_law(wrnn_stream_t *s, int on) {
    if (!s || !s->h) return WRNN_EINVAL;
    if (!s->raw) return fail(s->h, WRNN_EINVAL, "mu-law expansion belongs to RAW sessions: this session is MoL");
    if (s->primed || s->fin || s->dead)
        return fail(s->h, WRNN_EINVAL, "wrnn_stream_mu_law is set before the session's first push");
    s->mu_law = on != 0;
    return WRNN_OK;
}

int wrnn_stream_open_wide(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                          const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                          uint64_t seed, int64_t row_offset, wrnn_stream_t **out) {
    return stream_open(h, ucfg, mcfg, melresnet_packed, U, total_frames, noise, noise_steps, seed, row_offset, out, true);
}

// One persistent launch per time chunk of the steps [t_begin, t_end) of a push, through the kernel's
// own launcher; `last`: the utterance ends at t_end.
template <typename Args, typename Slab>
static int stream_launches(wrnn_stream *s, int t_begin, int t_end, bool last, const Slab &slab,
                           hipError_t (*launch)(const Args &, hipStream_t), hipStream_t st) {
    wrnn_t *h = s->h;
    const double budget = terms_budget_floats();
    const int Lc_max = (int)std::max(1.0, std::min((double)(t_end - t_begin), budget / ((double)s->U * s->N) - 1.0));
    HIP_TRY(h, ensure(s->d_T, s->T_cap, (size_t)(Lc_max + 1) * s->U * s->N));
    for (int t0 = t_begin; t0 < t_end; t0 += Lc_max) {
        const int Lc = std::min(Lc_max, t_end - t0);
        // one step ahead (the kernels prefetch the terms of t + 1), unless the utterance ends there
        const int rows = last ? std::min(Lc + 1, t_end - t0) : Lc + 1;
        HIP_TRY(h, launch_terms_interp_win(s->FT.buf[s->FT.cur], (int)s->FT.base, s->AT.buf[s->AT.cur], (int)s->AT.base,
                                           s->d_coef, s->d_T, s->N, s->U, s->hop, s->nJ, t0, rows, st));
        HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
        Args a{};
        a.slab = h->d_xslab;
        a.terms = s->d_T;
        a.noise = s->noise;
        a.out = s->d_y[s->y_cur];
        a.state = s->d_state;
        a.xg = s->d_xg;
        a.members = h->d_members;
        a.ctl = h->d_ctl;
        a.seed = s->seed;
        a.row0 = s->row_offset;
        a.timeout_ticks = h->timeout_ticks;
        // the end is in sight only in the last push; until then the loop horizon lies past every chunk
        a.L = last ? t_end : INT_MAX;
        a.windowed = 1;
        a.nz_hor = s->noise ? s->noise_steps : INT_MAX;
        a.out_ld = s->y_ld[s->y_cur];
        a.out_t0 = s->y_t0;
        a.t0 = t0;
        a.Lc = Lc;
        a.Bt = s->U;
        a.b0 = 0;
        a.nb = s->U;
        a.s = slab;
        a.dbg = nullptr;
        a.dbg_steps = 0;
        HIP_TRY(h, launch(a, st));
    }
    return WRNN_OK;
}

// One member's share of a push (wrnn_stream_push: the group of one), in three parts: the argument
// checks (stream_check: nothing queued, nothing changed), the conditioning of the new frames and the
// sample window of the steps that became runnable (stream_prepare), then — after the persistent
// launch(es) of those steps — the float64 post and the counters (stream_finish).
struct StreamPush {
    const float *mel = nullptr;
    int n = 0;
    bool final = false;
    double *wave = nullptr;
    int cap = 0;
    long long S_new = 0, Au_new = 0;   // the counts after this push
    int S_old = 0, m = 0, R_new = 0, A_new = 0;
};

static int stream_check(wrnn_stream *s, StreamPush &p) {
    wrnn_t *h = s->h;
    // the slabs a push launches with are the handle's: after a reload they hold another model (or
    // another kernel's layout), and the session's state belongs to the one it was opened with
    if (s->loads != h->loads) {
        s->dead = true;
        return fail(h, WRNN_EINVAL, "the handle's weights were loaded again (wrnn_set_weights) after this session was "
                                    "opened: a session binds the weights it was opened with; close it and open a new one");
    }
    if (s->dead) return fail(h, WRNN_EINVAL, "the session failed in an earlier push: close it");
    if (s->fin) return fail(h, WRNN_EINVAL, "push after the final one: the session is finished");
    if (p.n < 0 || (p.n > 0 && !p.mel) || p.cap < 0) return fail(h, WRNN_EINVAL, "need n >= 0, mel when n > 0, cap >= 0");
    std::string msg;
    if (int rc = stream_counts(s->hop, s->pad + 1, (long long)s->R + p.n, p.final, s->T_known, &p.S_new, &p.Au_new, &msg))
        return fail(h, rc, msg);
    p.m = (int)(p.Au_new - s->audio);
    if (p.m > 0 && (!p.wave || p.cap < p.m))
        return fail(h, WRNN_EINVAL, "this push emits " + std::to_string(p.m) + " samples per utterance: wave holds " +
                                        std::to_string(p.wave ? p.cap : 0));
    if (s->noise && p.S_new > s->noise_steps)
        return fail(h, WRNN_EINVAL, "the injected draws cover " + std::to_string(s->noise_steps) + " steps, the loop reaches " +
                                        std::to_string(p.S_new));
    p.S_old = s->steps;
    return WRNN_OK;
}

// Room in the not-yet-emitted sample window for the steps up to S_new: when the live buffer is too
// short the held-back samples move to the front of the other one, which is then the live one.
static int stream_sample_window(wrnn_stream *s, long long S_new, hipStream_t st) {
    wrnn_t *h = s->h;
    const int U = s->U;
    const int S_old = s->steps;
    if (S_new > S_old) {
        const int held = S_old - s->audio;   // samples run but still held back
        if ((int)S_new - s->y_t0 > s->y_ld[s->y_cur]) {
            const int o = 1 - s->y_cur, need = (int)S_new - s->audio;
            if ((size_t)need * U > s->y_cap[o]) HIP_TRY(h, ensure(s->d_y[o], s->y_cap[o], (size_t)2 * need * U));
            s->y_ld[o] = (int)(s->y_cap[o] / U);
            if (held > 0)
                HIP_TRY(h, hipMemcpy2DAsync(s->d_y[o], (size_t)s->y_ld[o] * 4, s->d_y[s->y_cur] + (s->audio - s->y_t0),
                                            (size_t)s->y_ld[s->y_cur] * 4, (size_t)held * 4, U, hipMemcpyDeviceToDevice, st));
            s->y_cur = o;
            s->y_t0 = s->audio;
        }
    }
    return WRNN_OK;
}

static int stream_prepare(wrnn_stream *s, StreamPush &p, hipStream_t st) {
    wrnn_t *h = s->h;
    const int U = s->U, feat = h->cfg.feat_dims, A4 = h->CD - feat, KX = h->KXc, N = s->N, pad = s->pad;
    const int jhi = s->jlo + s->nJ - 1;
    const float *mel = p.mel;
    const int n = p.n;
    const bool final = p.final;
    const long long S_new = p.S_new;
    // From here on work is queued and the session's stores advance: a failure on the way, whatever
    // its code, leaves them out of step with the frame counts, so the session is dead until the end
    s->dead = true;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = blas_on(h, st)) return rc;
    const float one = 1.0f, zero = 0.0f;
    // C[m][N] = W·X for `frames` frame records in d_frec, through the path's terms GEMM
    XcdmGemm wgemms[3];
    if (s->wide) xcdm_terms_gemms(*h, wgemms);
    auto gemm = [&](int frames, float ones, float *C) -> int {
        HIP_TRY(h, ensure(s->d_X, s->X_cap, (size_t)frames * U * KX));
        if (s->wide) {   // the many-row kernel's three segmented GEMMs on the split input (generate_xcdm)
            HIP_TRY(h, launch_pack_cond_input(s->d_frec, h->CD, U, 0, U, 0, frames, KX, s->d_X, st,
                                              h->cfg.feat_dims + h->cfg.aux_dims, ones));
            for (const XcdmGemm &g : wgemms)
                if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, g.rows, frames * U, g.k, &one,
                                  h->d_xmWt + (size_t)g.row0 * KX + g.col0, KX, s->d_X + g.col0, KX, &zero, C + g.row0,
                                  N) != rocblas_status_success)
                    return fail(h, WRNN_EHIP, "rocblas_sgemm (frame terms) failed");
            return WRNN_OK;
        }
        HIP_TRY(h, launch_pack_cond_input(s->d_frec, h->CD, U, 0, U, 0, frames, KX, s->d_X, st, 0, ones));
        if (rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, N, frames * U, KX, &one, h->d_xWt,
                          KX, s->d_X, KX, &zero, C, N) != rocblas_status_success)
            return fail(h, WRNN_EHIP, "rocblas_sgemm (frame terms) failed");
        return WRNN_OK;
    };
    const int R_old = s->R, R_new = R_old + n;
    const long long keep_f = s->steps / s->hop;   // the frame of the next loop step: rows behind it are done with
    HIP_TRY(h, ensure(s->d_frec, s->frec_cap, (size_t)(std::max(n, 1) + pad) * U * h->CD));
    if (!s->primed) {   // the zero FT rows of the mel frames before frame 0
        if (s->jlo < 0) {
            if (int rc = win_reserve(h, s->FT, 0, -s->jlo, st)) return rc;
            HIP_TRY(h, hipMemsetAsync(s->FT.at(0), 0, (size_t)(-s->jlo) * s->FT.row * sizeof(float), st));
            s->FT.end = -s->jlo;
        }
        s->primed = true;
    }
    // aux frames that became computable: frame f needs the mel up to f + pad (zeros once the end is known)
    const int A_new = final ? R_new : std::max(s->A, R_new - pad);
    const int Tw = A_new - s->A, wn = Tw > 0 ? Tw + 2 * pad : 0;
    if (n > 0 || Tw > 0) {
        HIP_TRY(h, ensure(s->d_win, s->win_cap, (size_t)std::max(1, wn) * U * feat));
        HIP_TRY(h, launch_stream_mel_window(s->d_tail[s->tail_cur], mel, U, feat, n, R_old, 2 * pad, s->A - pad, wn,
                                            s->d_win, s->d_tail[1 - s->tail_cur], st));
        s->tail_cur = 1 - s->tail_cur;
    }
    // FT rows of the new mel frames (row i = frame − jlo), and zero rows past the last frame
    const int ft_zero = final ? std::max(0, jhi) : 0;
    if (n > 0 || ft_zero > 0) {
        if (int rc = win_reserve(h, s->FT, keep_f, n + ft_zero, st)) return rc;
        if (n > 0) {
            HIP_TRY(h, launch_frame_cond(mel, nullptr, U, feat, A4, n, n, 0, 0, s->d_frec, st));
            if (int rc = gemm(n, 0.0f, s->FT.at(s->FT.end))) return rc;
            s->FT.end += n;
        }
        if (ft_zero > 0) {
            HIP_TRY(h, hipMemsetAsync(s->FT.at(s->FT.end), 0, (size_t)ft_zero * s->FT.row * sizeof(float), st));
            s->FT.end += ft_zero;
        }
    }
    if (Tw > 0) {
        HIP_TRY(h, ensure(s->d_aux, s->aux_cap, (size_t)U * A4 * Tw));
        if (int rc = wrnn_melresnet(&s->mcfg, s->mr_packed, s->d_win, U, Tw, s->d_aux, st))
            return fail(h, rc, std::string("wrnn_melresnet: ") + wrnn_cond_last_error());
        if (int rc = win_reserve(h, s->AT, keep_f, Tw, st)) return rc;
        HIP_TRY(h, ensure(s->d_frec, s->frec_cap, (size_t)Tw * U * h->CD));
        HIP_TRY(h, launch_frame_cond(nullptr, s->d_aux, U, feat, A4, Tw, Tw, 0, 1, s->d_frec, st));
        if (int rc = gemm(Tw, 1.0f, s->AT.at(s->AT.end))) return rc;
        s->AT.end += Tw;
    }
    // the loop over the steps that became runnable, into the not-yet-emitted sample window
    if (int rc = stream_sample_window(s, S_new, st)) return rc;
    p.R_new = R_new;
    p.A_new = A_new;
    return WRNN_OK;
}

static int stream_finish(wrnn_stream *s, const StreamPush &p, int *n_out, hipStream_t st) {
    wrnn_t *h = s->h;
    if (p.m > 0) {
        const int T = p.final ? p.R_new : s->T_known;
        HIP_TRY(h, launch_postprocess_stream(s->d_y[s->y_cur], s->U, s->y_ld[s->y_cur], s->y_t0, s->audio, p.m,
                                             T >= 0 ? (T - 1) * s->hop : -1, 20 * s->hop, s->mu_law ? 1 : 0,
                                             (double)(h->cfg.n_classes - 1), p.wave, p.cap, st));
    }
    s->R = p.R_new;
    s->A = p.A_new;
    s->steps = (int)p.S_new;
    s->audio = (int)p.Au_new;
    s->fin = p.final;
    s->dead = false;
    if (n_out) *n_out = p.m;
    return WRNN_OK;
}

// ---- rows sessions: a push -----------------------------------------------------------------------
// Refused before anything is queued: the session's rows must still be one row block of the partition
// its carried state was laid out for (WRNN_ROW_GROUPS / WRNN_ROWS_GRANULES are read at every call)
static int rows_check(wrnn_stream *s) {
    wrnn_t *h = s->h;
    RowsBlock k;
    if (int rc = rows_session_block(h, s->U, 1, &k)) return rc;
    if (k.Bl != s->U || k.ng != s->rows_ng || k.state_grp != s->rows_state_grp)
        return fail(h, WRNN_EINVAL, "the multi-row kernel's partition for this session's rows changed since it was opened "
                                    "(WRNN_ROW_GROUPS): its carried state has the other layout");
    return WRNN_OK;
}

// stream_prepare for a rows session: the mel tail and the new frames, MelResNet on the frames whose
// aux became computable, the aux frames the steps still to run read, then the per-sample records of
// the newly runnable steps [S_old, S_new) (wrnn_upsample_pack_window) and room for their samples.
static int rows_prepare(wrnn_stream *s, StreamPush &p, hipStream_t st) {
    wrnn_t *h = s->h;
    const int U = s->U, feat = h->cfg.feat_dims, A4 = h->CD - feat, pad = s->pad, n = p.n;
    s->dead = true;   // as stream_prepare: from here on the session's stores advance
    HIP_TRY(h, hipSetDevice(h->device));
    const int R_old = s->R, R_new = R_old + n, A_old = s->A;
    const int A_new = p.final ? R_new : std::max(A_old, R_new - pad);
    const int Tw = A_new - A_old, wn = Tw > 0 ? Tw + 2 * pad : 0;
    const int S_old = s->steps, ns = (int)p.S_new - S_old;
    const int T = p.final ? R_new : s->T_known;
    int mlo = 0, mhi = 0, alo = 0, ahi = 0;
    if (ns > 0) {
        if (int rc = wrnn_upsample_window_frames(&s->ucfg, T, S_old, ns, &mlo, &mhi, &alo, &ahi))
            return fail(h, rc, std::string("upsample window: ") + wrnn_cond_last_error());
        if (mhi > R_new || (mhi > mlo && mlo < R_old - s->mel_keep) || ahi > A_new || alo < A_old - s->aux_keep)
            return fail(h, WRNN_EINVAL, "rows session: the steps of this push read frames the session does not hold");
    }
    const int nm = mhi - mlo, na = ahi - alo;
    if (n > 0 || Tw > 0 || ns > 0) {
        // both windows come from the same tail and the same new frames, and leave the same new tail
        HIP_TRY(h, ensure(s->d_win, s->win_cap, (size_t)std::max(1, wn) * U * feat));
        HIP_TRY(h, ensure(s->d_mwin, s->mwin_cap, (size_t)std::max(1, nm) * U * feat));
        HIP_TRY(h, launch_stream_mel_window(s->d_tail[s->tail_cur], p.mel, U, feat, n, R_old, s->mel_keep, A_old - pad, wn,
                                            s->d_win, s->d_tail[1 - s->tail_cur], st));
        if (nm > 0)
            HIP_TRY(h, launch_stream_mel_window(s->d_tail[s->tail_cur], p.mel, U, feat, n, R_old, s->mel_keep, mlo, nm,
                                                s->d_mwin, s->d_tail[1 - s->tail_cur], st));
        s->tail_cur = 1 - s->tail_cur;
    }
    if (Tw > 0) {
        HIP_TRY(h, ensure(s->d_aux, s->aux_cap, (size_t)U * A4 * Tw));
        if (int rc = wrnn_melresnet(&s->mcfg, s->mr_packed, s->d_win, U, Tw, s->d_aux, st))
            return fail(h, rc, std::string("wrnn_melresnet: ") + wrnn_cond_last_error());
    }
    if (Tw > 0 || na > 0) {   // the aux window of the steps, and the aux tail behind the newest frame
        HIP_TRY(h, ensure(s->d_awin, s->awin_cap, (size_t)std::max(1, na) * U * A4));
        HIP_TRY(h, launch_stream_mel_window(s->d_atail[s->atail_cur], s->d_aux, U, A4, Tw, A_old, s->aux_keep, alo, na,
                                            s->d_awin, s->d_atail[1 - s->atail_cur], st));
        s->atail_cur = 1 - s->atail_cur;
    }
    if (ns > 0) {
        HIP_TRY(h, ensure(s->d_cond, s->cond_cap, (size_t)ns * U * h->CD));
        if (int rc = wrnn_upsample_pack_window(&s->ucfg, s->d_mwin, mlo, nm, s->d_awin, alo, na, T, U, S_old, ns, s->d_cond, st))
            return fail(h, rc, std::string("upsample_pack_window: ") + wrnn_cond_last_error());
    }
    if (int rc = stream_sample_window(s, p.S_new, st)) return rc;
    p.R_new = R_new;
    p.A_new = A_new;
    return WRNN_OK;
}

// The steps [S_old, S_new) through generate_rows' own pieces: the same block choices for the
// session's rows, the hop areas zeroed once per push, one terms GEMM and one persistent launch per
// time chunk.  State, records and sample window are the session's; t0 is the absolute step.
static int rows_launches(wrnn_stream *s, const StreamPush &p, hipStream_t st) {
    wrnn_t *h = s->h;
    const int ns = (int)p.S_new - p.S_old;
    const bool grouped = rows_grouped(*h, s->U);
    PartScope ps(*h, h->g2, grouped);
    if (int rc = rows_hop_areas(h)) return rc;
    if (int rc = blas_on(h, st)) return rc;
    RowsBlock k;
    if (int rc = rows_block(h, grouped, s->U, ns, &k)) return rc;
    if (k.Bl != s->U || k.ng != s->rows_ng || k.state_grp != s->rows_state_grp)
        return fail(h, WRNN_EINVAL, "rows session: the partition changed during the push");
    if (grow(h, h->d_X, h->X_cap, (size_t)k.Lc_max * k.Bg * k.KXg) || grow(h, h->d_T, h->T_cap, k.ng * k.T_grp) ||
        grow(h, h->d_act, h->act_cap, k.ng * k.act_grp))
        return WRNN_EHIP;
    // the handle's hop areas carry step tags: whatever a one-shot call or another session left there
    // since the last push must not satisfy a poll of this one
    if (int rc = rows_reset(h, k, true, st)) return rc;
    set_last_path(h, h->rows_gw ? 9 : (int)P_ROWS);
    note_row_block(h, k.ng, k.Bl, k.TB);
    RowsRun r{};
    r.cond = s->d_cond;
    r.cond_t0 = p.S_old;
    r.Bt = s->U;
    r.b0 = 0;
    r.noise = s->noise;
    // the kernel writes row b, step t at out[b·out_ld + t]: column t − y_t0 of the session's window
    r.out = s->d_y[s->y_cur] - s->y_t0;
    r.out_ld = s->y_ld[s->y_cur];
    r.labels = nullptr;
    r.state = s->d_state;
    r.seed = s->seed;
    r.row_offset = s->row_offset;
    for (int t0 = p.S_old; t0 < (int)p.S_new; t0 += k.Lc_max)
        if (int rc = rows_chunk(h, k, r, t0, std::min(k.Lc_max, (int)p.S_new - t0), st)) return rc;
    return WRNN_OK;
}

// ---- wide groups: the members' rows through the many-row kernel's grouped instantiation ------------
void wrnn::host::push_launches(std::vector<WideLaunch> &ls, long long prev, long long c, int Lc_max, int rows) {
    for (long long off = prev; off < c; off += Lc_max) ls.push_back({(int)off, (int)std::min<long long>(Lc_max, c - off), rows});
}

int wrnn::host::emit_launches(const std::vector<WideLaunch> &ls, int *first, int *steps, int *rows, int cap) {
    for (size_t j = 0; j < ls.size() && (int)j < cap; ++j) {
        if (first) first[j] = ls[j].off;
        if (steps) steps[j] = ls[j].Lc;
        if (rows) rows[j] = ls[j].rows;
    }
    return (int)ls.size();
}

// The round plan of one push (host only): members with step counts n[i] (0: none) are cut into rounds
// at the distinct counts in ascending order — round r runs launch-local steps [cut[r − 1], cut[r]) of
// every member with n[i] ≥ cut[r] — and every round into launches of at most Lc_max steps.  The rows
// of a launch are the surviving members' rows in member order, compacted: launch row r sits on XCD
// r % 8, slot r / 8.  → (first step, steps, rows) per launch.
static std::vector<WideLaunch> wide_plan(const int *n, const int *U, int count, int Lc_max) {
    std::vector<int> cuts;
    for (int i = 0; i < count; ++i)
        if (n[i] > 0) cuts.push_back(n[i]);
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    std::vector<WideLaunch> ls;
    int prev = 0;
    for (int c : cuts) {
        int rows = 0;
        for (int i = 0; i < count; ++i)
            if (n[i] >= c) rows += U[i];
        push_launches(ls, prev, c, Lc_max, rows);
        prev = c;
    }
    return ls;
}

// Steps per persistent launch of a wide push: the WRNN_TERMS_MB budget over the floats of one step of
// all rows with a step to run, one step kept back for the look-ahead row of the terms.  MoL: the
// terms alone (the 11 uniforms are negligible beside them).  RAW: the terms and the kMRawNC draws.
static int wide_steps_per_launch(int rows, int longest, bool raw) {
    const int N = kXcdWgs * kMRing;
    const double budget = terms_budget_floats();
    const double per_step = raw ? (double)rows * (N + kMRawNC) : (double)rows * N;
    return (int)std::max(1.0, std::min((double)longest, budget / per_step - 1.0));
}

int wrnn_wide_steps_per_launch(int rows, int longest_steps, int raw) {
    if (rows < 1 || rows > kMRowsMax || longest_steps < 1)
        return cond_fail(WRNN_EINVAL, "need 1.." + std::to_string(kMRowsMax) + " rows and longest_steps >= 1");
    return wide_steps_per_launch(rows, longest_steps, raw != 0);
}

int wrnn_wide_plan(const int *steps, const int *rows, int count, int steps_per_launch, int *launch_first,
                   int *launch_steps, int *launch_rows, int cap) {
    if (!steps || !rows || count < 1 || steps_per_launch < 1) return cond_fail(WRNN_EINVAL, "need steps, rows, count >= 1 and steps_per_launch >= 1");
    int total = 0;
    for (int i = 0; i < count; ++i) {
        if (steps[i] < 0 || rows[i] < 1) return cond_fail(WRNN_EINVAL, "a member has steps >= 0 and rows >= 1");
        total += rows[i];
    }
    if (total > kMRowsMax) return cond_fail(WRNN_EINVAL, "a wide group has at most " + std::to_string(kMRowsMax) + " rows");
    return emit_launches(wide_plan(steps, rows, count, steps_per_launch), launch_first, launch_steps, launch_rows, cap);
}

// Row-table records that hold the `ntab` fold records of a folded list (frame_terms.h: FoldRow): they
// ride behind the row records in the same table, so one upload brings both
size_t wrnn::host::fold_tab_records(size_t ntab) { return (ntab * sizeof(FoldRow) + sizeof(XcdmRow) - 1) / sizeof(XcdmRow); }

// The row table sized for `ntab` records (StagedTable::reserve: the caller may rewrite the staging
// copy on return), and the member counters of the grouped launches.
int wrnn::host::wide_tab_reserve(wrnn_t *h, size_t ntab) {
    HIP_TRY(h, h->wtab.reserve(ntab));
    if (!h->d_members) HIP_TRY(h, hipMalloc(&h->d_members, kXcds * sizeof(int)));
    return WRNN_OK;
}

// The launch loop of a wide push and of a wide list: the `ntab` records of wtab.h (the launches' row
// tables one after the other) go up once, then per launch one interpolation launch into the shared
// terms, one draws launch, the hop area reset, the member counters and one persistent launch.  The
// workspaces are grown already; nothing here waits on the stream.  `folds`: the rows are folds of a
// folded list — the table holds fold_tab_records(ntab) more records, the FoldRow of every row in
// table order, and the fold-aware interpolation takes the place of the windowed one.
int wrnn::host::wide_run_launches(wrnn_t *h, const std::vector<WideLaunch> &ls, size_t ntab, const float *d_coef, int hop,
                                  int nJ, bool raw, int K, hipStream_t st, bool folds) {
    const int N = kXcdWgs * kMRing;
    const FoldRow *d_folds = reinterpret_cast<const FoldRow *>(h->wtab.d + ntab);
    // ---- queuing begins
    HIP_TRY(h, h->wtab.upload(ntab + (folds ? fold_tab_records(ntab) : 0), st));
    HIP_TRY(h, hipMemsetAsync(h->d_ctl, 0, kCtlWords * sizeof(int), st));
    set_last_path(h, (int)P_XCDM);
    // wrnn_elapsed_ms: the loop share of this push (interpolation, draws, resets and persistent
    // launches of all its rounds), so a caller can split a tick into conditioning and loop
    HIP_TRY(h, hipEventRecord(h->ev0, st));
    size_t at = 0;
    for (const WideLaunch &l : ls) {
        const XcdmRow *tab = h->wtab.d + at;
        if (folds) HIP_TRY(h, launch_terms_interp_folds(tab, d_folds + at, d_coef, h->d_T, N, hop, nJ, l.rows, l.Lc, st));
        else HIP_TRY(h, launch_terms_interp_wide(tab, d_coef, h->d_T, N, hop, nJ, l.rows, l.Lc, st));
        at += (size_t)l.rows;
        HIP_TRY(h, launch_draws_wide(h->d_xmnoise, tab, l.rows, l.Lc, K, raw ? 0 : 1, st));
        // every packed hop element empty, every tag one no step carries (fatchord_xcdm.h)
        HIP_TRY(h, hipMemsetAsync(h->d_xmxg, 0xFF, (size_t)kXcds * kMXcdStride * 8, st));
        HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
        XcdmArgs a{};
        a.slab = h->d_xmslab;
        a.terms = h->d_T;
        a.noise = h->d_xmnoise;
        a.nz_ts = l.rows;
        a.nz_t0 = 0;
        a.nz_b0 = 0;
        a.xg = h->d_xmxg;
        a.members = h->d_members;
        a.ctl = h->d_ctl;
        a.timeout_ticks = h->timeout_ticks;
        a.t0 = 0;
        a.Lc = l.Lc;
        a.Bt = l.rows;
        a.nb = l.rows;
        a.s = h->xms;
        a.rows = tab;
        HIP_TRY(h, launch_xcdm_group(a, raw, st));
    }
    HIP_TRY(h, hipEventRecord(h->ev1, st));
    h->timed = true;
    return WRNN_OK;
}

// Per launch of the plan: the row table (uploaded once for the whole push), one interpolation launch
// into the shared terms, one draws launch, the hop area reset to all-ones (tags and slot parities
// restart at every launch), the membership counters, one persistent launch.  Nothing here outlives
// the launch on the handle: the terms, the draws and the hop area are rewritten before each one, the
// state lives in the sessions' records — so one-shot calls and narrow sessions may run in between.
static int wide_group_launches(wrnn_t *h, wrnn_stream *const *ss, const StreamPush *ps, int count, hipStream_t st) {
    std::vector<int> n(count), U(count);
    int rows = 0, longest = 0;
    for (int i = 0; i < count; ++i) {
        n[i] = (int)ps[i].S_new - ps[i].S_old;
        U[i] = ss[i]->U;
        if (n[i] > 0) {
            rows += U[i];
            longest = std::max(longest, n[i]);
        }
    }
    if (rows == 0) return WRNN_OK;
    const int N = kXcdWgs * kMRing;
    // a handle has one mode: every member draws the same width (MoL: 11 uniforms; RAW: one Exp(1) per class)
    const bool raw = ss[0]->raw;
    const int K = ss[0]->noise_k;
    const int Lc_max = wide_steps_per_launch(rows, longest, raw);
    const std::vector<WideLaunch> ls = wide_plan(n.data(), U.data(), count, Lc_max);
    size_t ntab = 0;
    for (const WideLaunch &l : ls) ntab += (size_t)l.rows;
    if (grow(h, h->d_T, h->T_cap, (size_t)(Lc_max + 1) * rows * N) ||
        grow(h, h->d_xmnoise, h->xmnoise_cap, (size_t)Lc_max * rows * K))
        return WRNN_EHIP;
    if (int rc = wide_tab_reserve(h, ntab)) return rc;
    size_t at = 0;
    for (const WideLaunch &l : ls) {
        for (int i = 0; i < count; ++i) {
            if (n[i] <= l.off) continue;   // done (or without a step in this push): the member takes no slot
            wrnn_stream *s = ss[i];
            const int t0 = ps[i].S_old + l.off;
            for (int u = 0; u < s->U; ++u) {
                XcdmRow r{};
                r.ft = s->FT.buf[s->FT.cur] + (size_t)u * N;
                r.at = s->AT.buf[s->AT.cur] + (size_t)u * N;
                r.fr_ld = (long long)s->U * N;
                r.noise = s->noise ? s->noise + ((size_t)t0 * s->U + u) * K : nullptr;
                r.noise_ld = (long long)s->U * K;
                r.seed = s->seed;
                r.prow = s->row_offset + u;
                r.out = s->d_y[s->y_cur] + (size_t)u * s->y_ld[s->y_cur] + (t0 - s->y_t0);
                r.state = s->d_state + (size_t)u * kXcdWgs * kMRowStateW;
                r.ft_base = (int)s->FT.base;
                r.at_base = (int)s->AT.base;
                r.t0 = t0;
                r.resume = t0 > 0;
                h->wtab.h[at++] = r;
            }
        }
    }
    if (at != ntab) return fail(h, WRNN_EINVAL, "wide group: the row tables do not match the plan");
    const wrnn_stream *s0 = ss[0];
    return wide_run_launches(h, ls, ntab, s0->d_coef, s0->hop, s0->nJ, raw, K, st);
}

// The group of one, through the launch-wide windowed kernel (wide sessions: the wide group of one)
int wrnn_stream_push(wrnn_stream_t *s, const float *mel, int n, int final, double *wave, int cap, int *n_out,
                     void *stream) {
    if (!s || !s->h) return WRNN_EINVAL;
    wrnn_t *h = s->h;
    hipStream_t st = (hipStream_t)stream;
    if (n_out) *n_out = 0;
    StreamPush p;
    p.mel = mel, p.n = n, p.final = final != 0, p.wave = wave, p.cap = cap;
    if (int rc = stream_check(s, p)) return rc;
    if (s->rows) {
        if (int rc = rows_check(s)) return rc;
        if (int rc = rows_prepare(s, p, st)) return rc;
    } else if (int rc = stream_prepare(s, p, st)) {
        return rc;
    }
    if (p.S_new > p.S_old) {
        HIP_TRY(h, hipMemsetAsync(h->d_ctl, 0, kCtlWords * sizeof(int), st));
        set_last_path(h, (int)s->path);  // the timing events stay the last wrnn_generate's (wrnn_elapsed_ms)
        int rc;
        if (s->rows) rc = rows_launches(s, p, st);
        else if (s->wide) rc = wide_group_launches(h, &s, &p, 1, st);
        else if (s->path == P_XCD) rc = stream_launches<XcdArgs>(s, p.S_old, (int)p.S_new, p.final, h->xs, launch_xcd, st);
        else rc = stream_launches<XcdsArgs>(s, p.S_old, (int)p.S_new, p.final, h->xss, launch_xcds, st);
        if (rc) return rc;
    }
    return stream_finish(s, p, n_out, st);
}

// One persistent launch per time chunk for every member with steps to run: member i's rows take
// the XCDs after those of the members before it, each over its own window (the kernels' kGrp
// instantiation).  The terms budget is shared by all those rows; round j runs chunk j of every
// member that still has one.
template <typename GroupArgs, typename Slab>
static int group_launches(wrnn_t *h, wrnn_stream *const *ss, const StreamPush *ps, int count, const Slab &slab,
                          hipError_t (*launch)(const GroupArgs &, hipStream_t), hipStream_t st) {
    int rows = 0, longest = 0;
    for (int i = 0; i < count; ++i)
        if (ps[i].S_new > ps[i].S_old) {
            rows += ss[i]->U;
            longest = std::max(longest, (int)ps[i].S_new - ps[i].S_old);
        }
    if (rows == 0) return WRNN_OK;
    const int N = ss[0]->N;
    const double budget = terms_budget_floats();
    const int Lc_max = (int)std::max(1.0, std::min((double)longest, budget / ((double)rows * N) - 1.0));
    for (int i = 0; i < count; ++i)
        if (ps[i].S_new > ps[i].S_old) {
            const int steps = std::min(Lc_max, (int)ps[i].S_new - ps[i].S_old);
            HIP_TRY(h, ensure(ss[i]->d_T, ss[i]->T_cap, (size_t)(steps + 1) * ss[i]->U * N));
        }
    HIP_TRY(h, hipMemsetAsync(h->d_ctl, 0, kCtlWords * sizeof(int), st));
    set_last_path(h, (int)ss[0]->path);  // the timing events stay the last wrnn_generate's (wrnn_elapsed_ms)
    for (int off = 0; off < longest; off += Lc_max) {
        GroupArgs g{};
        g.a.slab = h->d_xslab;
        g.a.members = h->d_members;
        g.a.ctl = h->d_ctl;
        g.a.timeout_ticks = h->timeout_ticks;
        g.a.s = slab;
        g.a.windowed = 1;
        int k = 0;
        for (int i = 0; i < count; ++i) {
            wrnn_stream *s = ss[i];
            const int t0 = ps[i].S_old + off, t_end = (int)ps[i].S_new;
            if (t0 >= t_end) continue;   // no step (left) in this push: the member takes no XCD
            const int Lc = std::min(Lc_max, t_end - t0);
            const bool last = ps[i].final;
            // one step ahead (the kernels prefetch the terms of t + 1), unless the utterance ends there
            const int trows = last ? std::min(Lc + 1, t_end - t0) : Lc + 1;
            HIP_TRY(h, launch_terms_interp_win(s->FT.buf[s->FT.cur], (int)s->FT.base, s->AT.buf[s->AT.cur], (int)s->AT.base,
                                               s->d_coef, s->d_T, N, s->U, s->hop, s->nJ, t0, trows, st));
            for (int u = 0; u < s->U; ++u, ++k) {
                XcdRow &r = g.row[k];
                r.terms = s->d_T + (size_t)u * N;
                r.terms_ld = (long long)s->U * N;
                r.noise = s->noise ? s->noise + (size_t)u * 11 : nullptr;
                r.noise_ld = s->U * 11;
                r.seed = s->seed;
                r.row = s->row_offset + u;
                r.out = s->d_y[s->y_cur] + (size_t)u * s->y_ld[s->y_cur];
                r.out_t0 = s->y_t0;
                r.state = s->d_state + (size_t)u * kXcdWgs * s->state_w;
                r.xg = s->d_xg + (size_t)u * kXXcdStride;
                r.t0 = t0;
                r.Lc = Lc;
                // the end is in sight only in the last push; until then the loop horizon lies past every chunk
                r.L = last ? t_end : INT_MAX;
                r.nz_hor = s->noise ? s->noise_steps : INT_MAX;
            }
        }
        g.a.nb = k;
        HIP_TRY(h, hipMemsetAsync(h->d_members, 0, kXcds * sizeof(int), st));
        HIP_TRY(h, launch(g, st));
    }
    return WRNN_OK;
}

int wrnn_stream_push_group(wrnn_stream_t *const *sessions, int count, const float *const *mel, const int *n,
                           const int *final, double *const *wave, const int *cap, int *n_out, void *stream) {
    if (!sessions || count < 1 || !sessions[0] || !sessions[0]->h) return WRNN_EINVAL;
    wrnn_t *h = sessions[0]->h;
    hipStream_t st = (hipStream_t)stream;
    if (n_out)
        for (int i = 0; i < count; ++i) n_out[i] = 0;
    if (!n || !final || !cap) return fail(h, WRNN_EINVAL, "need n, final and cap for every member");
    // every member is checked before anything is queued for any of them
    int rows = 0;
    for (int i = 0; i < count; ++i) {
        if (!sessions[i]) return fail(h, WRNN_EINVAL, "member " + std::to_string(i) + " is null");
        if (sessions[i]->h != h) return fail(h, WRNN_EINVAL, "member " + std::to_string(i) + " belongs to another handle");
        for (int j = 0; j < i; ++j)
            if (sessions[j] == sessions[i])
                return fail(h, WRNN_EINVAL, "members " + std::to_string(j) + " and " + std::to_string(i) + " are the same session");
        if (sessions[i]->rows)
            return fail(h, WRNN_EINVAL, "member " + std::to_string(i) + ": a rows session advances alone: its kernel steps "
                                        "all rows in lock step");
        if (sessions[i]->path != sessions[0]->path)
            return fail(h, WRNN_EINVAL, "member " + std::to_string(i) + " runs another loop kernel than member 0");
        rows += sessions[i]->U;
    }
    const bool wide = sessions[0]->wide;
    if (wide) {
        if (rows > kMRowsMax)
            return fail(h, WRNN_EINVAL, "a wide group has at most " + std::to_string(kMRowsMax) + " rows (" +
                                            std::to_string(kMRowsXcd) + " per XCD): these members have " + std::to_string(rows));
        // one interpolation launch serves every member: they share one upsample cascade
        for (int i = 1; i < count; ++i) {
            const wrnn_stream *a = sessions[0], *b = sessions[i];
            bool same = a->hop == b->hop && a->nJ == b->nJ && a->jlo == b->jlo && a->pad == b->pad &&
                        a->ucfg.n_scales == b->ucfg.n_scales;
            for (int j = 0; same && j < a->ucfg.n_scales; ++j) same = a->taps[j] == b->taps[j];
            if (!same)
                return fail(h, WRNN_EINVAL, "member " + std::to_string(i) + " has another upsample cascade than member 0");
        }
    }
    if (!wide && rows > kXcds)
        return fail(h, WRNN_EINVAL, "a group has at most " + std::to_string(kXcds) + " rows (one per XCD): these members have " +
                                        std::to_string(rows));
    std::vector<StreamPush> ps(count);
    for (int i = 0; i < count; ++i) {
        StreamPush &p = ps[i];
        p.mel = mel ? mel[i] : nullptr, p.n = n[i], p.final = final[i] != 0;
        p.wave = wave ? wave[i] : nullptr, p.cap = cap[i];
        if (int rc = stream_check(sessions[i], p)) {
            const std::string why = h->err;
            return fail(h, rc, "member " + std::to_string(i) + ": " + why);
        }
    }
    // queuing begins: a failure from here on leaves the stores of the members already prepared out of
    // step with their counts, and the launch is shared, so it kills every member
    for (int i = 0; i < count; ++i) sessions[i]->dead = true;
    for (int i = 0; i < count; ++i)
        if (int rc = stream_prepare(sessions[i], ps[i], st)) return rc;
    int rc;
    if (wide) rc = wide_group_launches(h, sessions, ps.data(), count, st);
    else if (sessions[0]->path == P_XCD) rc = group_launches<XcdGroupArgs>(h, sessions, ps.data(), count, h->xs, launch_xcd_group, st);
    else rc = group_launches<XcdsGroupArgs>(h, sessions, ps.data(), count, h->xss, launch_xcds_group, st);
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (int rc2 = stream_finish(sessions[i], ps[i], n_out ? &n_out[i] : nullptr, st)) return rc2;
    return WRNN_OK;
}
