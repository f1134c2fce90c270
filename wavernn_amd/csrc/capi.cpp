// capi.cpp — host side of the C-ABI declared in include/wavernn_amd.h: the handle and its weights.
// wrnn_create lays the kernels' slabs and partitions out, wrnn_set_weights packs them from the
// reference state_dict tensors and uploads them; then check, query and destroy.  The rest of the
// host side: capi_loops.cpp (one-shot runners), capi_lists.cpp (list calls), capi_stream.cpp
// (streaming sessions); host_ctx.h is their common header.
#include "host_ctx.h"

using namespace wrnn;
using namespace wrnn::host;

// Layouts, partitions and packers: static unless another host file needs them (host_ctx.h)
namespace wrnn {
namespace host {

struct Need {
    const char *name;
    int64_t rows, cols;
};

static std::vector<Need> required(const wrnn_config &c) {
    if (c.mode == WRNN_MODE_DM) {   // deepmind_version.py:14-31
        const int64_t H = c.rnn_dims, S = H / 2, Q = c.n_classes;
        return {{"R.weight", 3 * H, H},      {"O1.weight", S, S},        {"O1.bias", S, 1},
                {"O2.weight", Q, S},         {"O2.bias", Q, 1},          {"O3.weight", S, S},
                {"O3.bias", S, 1},           {"O4.weight", Q, S},        {"O4.bias", Q, 1},
                {"I_coarse.weight", 3 * S, 2}, {"I_fine.weight", 3 * S, 3}, {"bias_u", H, 1},
                {"bias_r", H, 1},            {"bias_e", H, 1}};
    }
    const int64_t R = c.rnn_dims, F = c.fc_dims, A = c.aux_dims, M = c.feat_dims, NC = c.n_classes;
    return {{"I.weight", R, 1 + M + A},      {"I.bias", R, 1},
            {"rnn1.weight_ih_l0", 3 * R, R}, {"rnn1.weight_hh_l0", 3 * R, R},
            {"rnn1.bias_ih_l0", 3 * R, 1},   {"rnn1.bias_hh_l0", 3 * R, 1},
            {"rnn2.weight_ih_l0", 3 * R, R + A}, {"rnn2.weight_hh_l0", 3 * R, R},
            {"rnn2.bias_ih_l0", 3 * R, 1},   {"rnn2.bias_hh_l0", 3 * R, 1},
            {"fc1.weight", F, R + A},        {"fc1.bias", F, 1},
            {"fc2.weight", F, F + A},        {"fc2.bias", F, 1},
            {"fc3.weight", NC, F},           {"fc3.bias", NC, 1}};
}

static SlabLayout make_slab_layout(const wrnn_ctx &h) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    SlabLayout s{};
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    s.wih1 = take(3 * h.U * R);
    s.whh1 = take(3 * h.U * R);
    s.wih2 = take(3 * h.U * (R + A));
    s.whh2 = take(3 * h.U * R);
    s.bih1 = take(3 * h.U);
    s.bhh1 = take(3 * h.U);
    s.bih2 = take(3 * h.U);
    s.bhh2 = take(3 * h.U);
    s.w1 = take(h.UF * (R + A));
    s.b1 = take(h.UF);
    s.w2 = take(h.UF * (F + A));
    s.b2 = take(h.UF);
    s.w3 = take((mol ? NC : h.UC) * F);
    s.b3 = take(mol ? NC : h.UC);
    s.wi0 = take(R);
    s.total = o;
    return s;
}

// Pack workgroup w's rows: GRU gate rows (g·R + j) for owned units j, fc rows, fc3 rows.
static void pack_slab(const wrnn_ctx &h, int w, float *out) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    const SlabLayout &s = h.s;
    std::fill(out, out + s.total, 0.0f);
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    for (int u = 0; u < h.U; ++u) {
        const int j = w * h.U + u;
        if (j >= R) continue;
        for (int g = 0; g < 3; ++g) {
            const int src = g * R + j, dst = g * h.U + u;
            std::memcpy(out + s.wih1 + (size_t)dst * R, W("rnn1.weight_ih_l0") + (size_t)src * R, R * 4);
            std::memcpy(out + s.whh1 + (size_t)dst * R, W("rnn1.weight_hh_l0") + (size_t)src * R, R * 4);
            std::memcpy(out + s.wih2 + (size_t)dst * (R + A), W("rnn2.weight_ih_l0") + (size_t)src * (R + A),
                        (R + A) * 4);
            std::memcpy(out + s.whh2 + (size_t)dst * R, W("rnn2.weight_hh_l0") + (size_t)src * R, R * 4);
            out[s.bih1 + dst] = W("rnn1.bias_ih_l0")[src];
            out[s.bhh1 + dst] = W("rnn1.bias_hh_l0")[src];
            out[s.bih2 + dst] = W("rnn2.bias_ih_l0")[src];
            out[s.bhh2 + dst] = W("rnn2.bias_hh_l0")[src];
        }
    }
    for (int r = 0; r < h.UF; ++r) {
        const int j = w * h.UF + r;
        if (j >= F) continue;
        std::memcpy(out + s.w1 + (size_t)r * (R + A), W("fc1.weight") + (size_t)j * (R + A), (R + A) * 4);
        std::memcpy(out + s.w2 + (size_t)r * (F + A), W("fc2.weight") + (size_t)j * (F + A), (F + A) * 4);
        out[s.b1 + r] = W("fc1.bias")[j];
        out[s.b2 + r] = W("fc2.bias")[j];
    }
    if (mol) {
        std::memcpy(out + s.w3, W("fc3.weight"), (size_t)NC * F * 4);
        std::memcpy(out + s.b3, W("fc3.bias"), (size_t)NC * 4);
    } else {
        for (int r = 0; r < h.UC; ++r) {
            const int j = w * h.UC + r;
            if (j >= NC) continue;
            std::memcpy(out + s.w3 + (size_t)r * F, W("fc3.weight") + (size_t)j * F, F * 4);
            out[s.b3 + r] = W("fc3.bias")[j];
        }
    }
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    for (int j = 0; j < R; ++j) out[s.wi0 + j] = IW[(size_t)j * nin];
}

static RowsSlab make_rows_slab(const wrnn_ctx &h, int nbmax) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, NC = h.cfg.n_classes;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    const int dense = nbmax > 0 ? 0 : 1;
    RowsSlab s{};
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    s.wih2 = take(dense * 3 * h.rU * R);
    s.whh1 = take(dense * 3 * h.rU * R);
    s.whh2 = take(dense * 3 * h.rU * R);
    s.sp = take(9 * nbmax * 16);
    s.spc = take(9 * nbmax);
    s.spn = take(nbmax > 0 ? 9 : 0);
    s.nbmax = nbmax;
    s.w1 = take(h.rUF * R);
    s.w2 = take(h.rUF * F);
    if (!mol) {
        s.w3 = take(h.rUC * F);
        s.b3 = take(h.rUC);
    }
    s.bih1 = take(3 * h.rU);
    s.bhh1 = take(3 * h.rU);
    s.bih2 = take(3 * h.rU);
    s.bhh2 = take(3 * h.rU);
    s.q1 = take(3 * h.rU);
    s.q2 = take(3 * h.rU);
    s.q3 = take(h.rUF);
    s.body = o;          // everything before the MoL head: always LDS-resident
    if (mol) {           // the replicated 30-row head last, so a launch may leave it in HBM
        s.w3 = take(NC * F);
        s.b3 = take(NC);
    }
    s.total = o;
    return s;
}

// The three GRU matrices the rows kernel multiplies in the loop, as (tensor, row stride):
// W_ih2[:, :R] (stride R + A), W_hh1, W_hh2 (SparseMat order).
struct LoopMat {
    const float *w;
    int ld;
};
static void loop_mats(const wrnn_ctx &h, LoopMat (&m)[3]) {
    const int R = h.cfg.rnn_dims, A = h.cfg.aux_dims;
    m[SP_WIH2] = {h.w.at("rnn2.weight_ih_l0").data(), R + A};
    m[SP_WHH1] = {h.w.at("rnn1.weight_hh_l0").data(), R};
    m[SP_WHH2] = {h.w.at("rnn2.weight_hh_l0").data(), R};
}

static bool block_nonzero(const float *w, int ld, int r0, int c0) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (w[(size_t)(r0 + r) * ld + c0 + c] != 0.0f) return true;
    return false;
}

// Largest nonzero-block count of any gate block-row (4 rows) of the three loop matrices, and the
// overall block density; the rows kernel goes sparse when density <= 1/2.
static void block_stats(const wrnn_ctx &h, int *nbmax, double *density) {
    const int R = h.cfg.rnn_dims;
    LoopMat m[3];
    loop_mats(h, m);
    long long nz = 0, tot = 0;
    int mx = 0;
    for (int k = 0; k < 3; ++k)
        for (int rb = 0; rb < 3 * R; rb += 4) {
            int n = 0;
            for (int cb = 0; cb < R; cb += 4) n += block_nonzero(m[k].w, m[k].ld, rb, cb);
            nz += n;
            tot += R / 4;
            mx = std::max(mx, n);
        }
    *nbmax = mx;
    *density = tot ? (double)nz / tot : 1.0;
}

// x-column constants Q = W[:, :R]·W_I[:, 0] (fp32, sequential)
static float xcol_dot(const float *wrow, const float *IW, int nin, int R) {
    float acc = 0.0f;
    for (int k = 0; k < R; ++k) acc = std::fma(wrow[k], IW[(size_t)k * nin], acc);
    return acc;
}

static void pack_rows_slab(const wrnn_ctx &h, int w, float *out) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    const RowsSlab &s = h.rs;
    const int U = h.rU, UF = h.rUF, UC = h.rUC;
    std::fill(out, out + s.total, 0.0f);
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    for (int u = 0; u < U; ++u) {
        const int j = w * U + u;
        if (j >= R) continue;
        for (int g = 0; g < 3; ++g) {
            const int src = g * R + j, dst = g * U + u;
            const float *ih1 = W("rnn1.weight_ih_l0") + (size_t)src * R;
            const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)src * (R + A);
            if (s.nbmax == 0) {
                std::memcpy(out + s.wih2 + (size_t)dst * R, ih2, R * 4);
                std::memcpy(out + s.whh1 + (size_t)dst * R, W("rnn1.weight_hh_l0") + (size_t)src * R, R * 4);
                std::memcpy(out + s.whh2 + (size_t)dst * R, W("rnn2.weight_hh_l0") + (size_t)src * R, R * 4);
            }
            out[s.bih1 + dst] = W("rnn1.bias_ih_l0")[src];
            out[s.bhh1 + dst] = W("rnn1.bias_hh_l0")[src];
            out[s.bih2 + dst] = W("rnn2.bias_ih_l0")[src];
            out[s.bhh2 + dst] = W("rnn2.bias_hh_l0")[src];
            out[s.q1 + dst] = xcol_dot(ih1, IW, nin, R);
            out[s.q2 + dst] = xcol_dot(ih2, IW, nin, R);
        }
    }
    if (s.nbmax > 0) {   // this workgroup's block-row (units 4w..4w+3) of each gate, nonzero blocks only
        LoopMat m[3];
        loop_mats(h, m);
        int *col = reinterpret_cast<int *>(out + s.spc);
        int *cnt = reinterpret_cast<int *>(out + s.spn);
        for (int k = 0; k < 3; ++k)
            for (int g = 0; g < 3; ++g) {
                const int r0 = g * R + 4 * w, sl = k * 3 + g;
                int n = 0;
                for (int cb = 0; cb < R; cb += 4) {
                    if (!block_nonzero(m[k].w, m[k].ld, r0, cb)) continue;
                    float *blk = out + s.sp + ((size_t)sl * s.nbmax + n) * 16;
                    for (int r = 0; r < 4; ++r)
                        for (int c = 0; c < 4; ++c) blk[r * 4 + c] = m[k].w[(size_t)(r0 + r) * m[k].ld + cb + c];
                    col[sl * s.nbmax + n] = cb / 4;
                    ++n;
                }
                cnt[sl] = n;
            }
    }
    for (int r = 0; r < UF; ++r) {
        const int j = w * UF + r;
        if (j >= F) continue;
        const float *w1 = W("fc1.weight") + (size_t)j * (R + A);
        std::memcpy(out + s.w1 + (size_t)r * R, w1, R * 4);
        std::memcpy(out + s.w2 + (size_t)r * F, W("fc2.weight") + (size_t)j * (F + A), F * 4);
        out[s.q3 + r] = xcol_dot(w1, IW, nin, R);
    }
    if (mol) {
        std::memcpy(out + s.w3, W("fc3.weight"), (size_t)NC * F * 4);
        std::memcpy(out + s.b3, W("fc3.bias"), (size_t)NC * 4);
    } else {
        for (int r = 0; r < UC; ++r) {
            const int j = w * UC + r;
            if (j >= NC) continue;
            std::memcpy(out + s.w3 + (size_t)r * F, W("fc3.weight") + (size_t)j * F, F * 4);
            out[s.b3 + r] = W("fc3.bias")[j];
        }
    }
}

// Weights of the conditioning-terms GEMM: row w·NT + k of [G·NT][KX] against X = [cI | a2 a3 a4 | 1 0 0 0]
static void pack_terms_weights(const wrnn_ctx &h, float *Wt) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, U = h.rU, UF = h.rUF, KX = h.KX;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    std::fill(Wt, Wt + (size_t)h.rG * h.NT * KX, 0.0f);
    for (int w = 0; w < h.rG; ++w)
        for (int k = 0; k < 6 * U + 2 * UF; ++k) {
            float *row = Wt + ((size_t)w * h.NT + k) * KX;
            if (k < 6 * U) {
                const int kk = k % (3 * U), g = kk / U, j = w * U + kk % U;
                if (j >= R) continue;
                if (k < 3 * U) {
                    std::memcpy(row, W("rnn1.weight_ih_l0") + (size_t)(g * R + j) * R, R * 4);
                } else {
                    const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)(g * R + j) * (R + A);
                    std::memcpy(row, ih2, R * 4);
                    std::memcpy(row + R, ih2 + R, A * 4);                       // a2
                }
            } else if (k < 6 * U + UF) {
                const int r = w * UF + (k - 6 * U);
                if (r >= F) continue;
                const float *w1 = W("fc1.weight") + (size_t)r * (R + A);
                std::memcpy(row, w1, R * 4);
                std::memcpy(row + R + A, w1 + R, A * 4);                        // a3
                row[R + 3 * A] = W("fc1.bias")[r];
            } else {
                const int r = w * UF + (k - 6 * U - UF);
                if (r >= F) continue;
                std::memcpy(row + R + 2 * A, W("fc2.weight") + (size_t)r * (F + A) + F, A * 4);   // a4
                row[R + 3 * A] = W("fc2.bias")[r];
            }
        }
}

static void fold_ci_row(const wrnn_ctx &h, const float *w, float *dst);

// MoL: the same slots against the composed input X' = [mel | a1 | a2 | a3 | a4 | 1 0 0 0]
// (KXc = CD + 4) — the I layer folded into the W_ih1 / W_ih2 / fc1 rows in fp64 (fold_ci_row,
// as the XCD kernels' terms), so the GEMM needs no cI and runs at depth 212 instead of R + 3A + 4
// (2.9x less work at rnn 512).  RAW keeps the cI GEMM (its labels are checked bit-exact).
bool rows_terms_composed(const wrnn_ctx &h) { return h.cfg.mode == WRNN_MODE_MOL; }
int rows_terms_kx(const wrnn_ctx &h) { return rows_terms_composed(h) ? h.KXc : h.KX; }

static void pack_terms_weights_composed(const wrnn_ctx &h, float *Wt) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, M = h.cfg.feat_dims, A = h.cfg.aux_dims, U = h.rU, UF = h.rUF;
    const int KX = h.KXc;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    std::fill(Wt, Wt + (size_t)h.rG * h.NT * KX, 0.0f);
    for (int w = 0; w < h.rG; ++w)
        for (int k = 0; k < 6 * U + 2 * UF; ++k) {
            float *row = Wt + ((size_t)w * h.NT + k) * KX;
            if (k < 6 * U) {
                const int kk = k % (3 * U), g = kk / U, j = w * U + kk % U;
                if (j >= R) continue;
                if (k < 3 * U) {
                    fold_ci_row(h, W("rnn1.weight_ih_l0") + (size_t)(g * R + j) * R, row);
                } else {
                    const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)(g * R + j) * (R + A);
                    fold_ci_row(h, ih2, row);
                    for (int a = 0; a < A; ++a) row[M + A + a] += ih2[R + a];                   // a2
                }
            } else if (k < 6 * U + UF) {
                const int r = w * UF + (k - 6 * U);
                if (r >= F) continue;
                const float *w1 = W("fc1.weight") + (size_t)r * (R + A);
                fold_ci_row(h, w1, row);
                for (int a = 0; a < A; ++a) row[M + 2 * A + a] += w1[R + a];                    // a3
                row[h.CD] += W("fc1.bias")[r];
            } else {
                const int r = w * UF + (k - 6 * U - UF);
                if (r >= F) continue;
                for (int a = 0; a < A; ++a) row[M + 3 * A + a] = W("fc2.weight")[(size_t)r * (F + A) + F + a];   // a4
                row[h.CD] = W("fc2.bias")[r];
            }
        }
}

size_t rows_lds_bytes(const wrnn_ctx &h, int B, int TB, bool head_lds) {
    const int slab = h.rows_gw ? 0 : head_lds ? h.rs.total : h.rs.body;
    return (size_t)rows_lds_layout(slab, B, TB, h.cfg.rnn_dims, h.cfg.fc_dims,
                                   h.cfg.n_classes, h.NK, h.rU, h.rUF, h.rG)
               .total * sizeof(float);
}

// (Re)derive the rows-kernel partition: dense = the latency kernel's; sparse = one 4-unit
// block-row per workgroup (G = R / 4).  Sets rows_ok.
static void set_rows_partition(wrnn_ctx &h, int nbmax) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    h.sparse = nbmax > 0;
    if (h.sparse) {
        h.rU = 4;
        h.rG = R / 4;
    } else {
        h.rU = h.U;
        h.rG = h.G;
    }
    h.rUF = (F + h.rG - 1) / h.rG;
    h.rUC = mol ? 0 : (h.cfg.n_classes + h.rG - 1) / h.rG;
    h.NT = rows_terms(h.rU, h.rUF);
    h.rs = make_rows_slab(h, nbmax);
    h.rows_gw = false;
    h.rows_ok = rows_tile_for(h, 1) > 0;
    // a sparse slab sized by one crowded block-row (W_hh pruned alone: nbmax = R / 4) may not fit
    // beside one row of state where the dense layout, resident or streamed, does: take that one
    if (!h.rows_ok && nbmax > 0) return set_rows_partition(h, 0);
    // dense weights beyond the grid's LDS: the same kernel with the slab streamed from HBM
    if (!h.rows_ok && nbmax == 0) {
        h.rows_gw = true;
        h.rows_ok = rows_tile_for(h, 1) > 0;
    }
}

// Largest tile (<= 16 rows; up to 32 with the MoL head left in HBM) that fits next to B rows of
// state; 0 if none does
int rows_tile_for(const wrnn_ctx &h, int B, bool head_lds) {
    for (int tb = std::min(B, head_lds ? 16 : 32); tb >= 1; --tb)
        if (rows_lds_bytes(h, B, tb, head_lds) <= (size_t)h.max_lds) return tb;
    return 0;
}

void swap_part(wrnn_ctx &h, RowsPart &p) {
    std::swap(h.rs, p.rs);
    std::swap(h.rU, p.rU);
    std::swap(h.rG, p.rG);
    std::swap(h.rUF, p.rUF);
    std::swap(h.rUC, p.rUC);
    std::swap(h.NT, p.NT);
    std::swap(h.rows_ok, p.ok);
    std::swap(h.d_rslab, p.d_slab);
    std::swap(h.d_Wt, p.d_Wt);
}


// The two-group partition: dense weights over G/2 workgroups (G even)
static void set_group_partition(wrnn_ctx &h) {
    h.g2 = RowsPart{};
    if (h.G % 2 || h.G < 8 || h.rows_gw) return;
    RowsPart flat{};
    swap_part(h, flat);   // h.r* empty, flat holds the current partition
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims;
    const bool mol = h.cfg.mode == WRNN_MODE_MOL;
    h.rG = h.G / 2;
    h.rU = (R + h.rG - 1) / h.rG;
    h.rUF = (F + h.rG - 1) / h.rG;
    h.rUC = mol ? 0 : (h.cfg.n_classes + h.rG - 1) / h.rG;
    h.NT = rows_terms(h.rU, h.rUF);
    h.rs = make_rows_slab(h, 0);
    h.rows_ok = rows_tile_for(h, 16, false) >= 4;
    swap_part(h, flat);   // h.r* = flat again, `flat` = the group partition
    h.g2 = flat;
}

// ------------------------------------------------------------------ deepmind_version packing
static DmSlab make_dm_slab(const wrnn_ctx &h) {
    const int H = h.cfg.rnn_dims, S = H / 2;
    DmSlab s{};
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    s.rw = take(6 * h.dmU * H);
    s.o1 = take(h.dmUO * S);
    s.o1b = take(h.dmUO);
    s.o3 = take(h.dmUO * S);
    s.o3b = take(h.dmUO);
    s.o2 = take(h.dmUO2 * S);
    s.o2b = take(h.dmUO2);
    s.o4 = take(h.dmUO2 * S);
    s.o4b = take(h.dmUO2);
    s.ic = take(3 * h.dmU * 2);
    s.if_ = take(3 * h.dmU * 3);
    s.bu = take(2 * h.dmU);
    s.br = take(2 * h.dmU);
    s.be = take(2 * h.dmU);
    s.total = o;
    return s;
}

// Workgroup w: coarse units j = w·U + u and fine units S + j; R rows g·H + half·S + j (g = u, r, e,
// the split of deepmind_version.py:116-119); output rows w·UO + r of O1/O3, w·UO2 + r of O2/O4.
static void pack_dm_slab(const wrnn_ctx &h, int w, float *out) {
    const int H = h.cfg.rnn_dims, S = H / 2, Q = h.cfg.n_classes, U = h.dmU;
    const DmSlab &s = h.ds;
    std::fill(out, out + s.total, 0.0f);
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    for (int u = 0; u < U; ++u) {
        const int j = w * U + u;
        if (j >= S) continue;
        for (int half = 0; half < 2; ++half)
            for (int g = 0; g < 3; ++g) {
                std::memcpy(out + s.rw + (size_t)((half * 3 + g) * U + u) * H,
                            W("R.weight") + (size_t)(g * H + half * S + j) * H, H * 4);
                const float *bias = W(g == 0 ? "bias_u" : g == 1 ? "bias_r" : "bias_e");
                out[(g == 0 ? s.bu : g == 1 ? s.br : s.be) + half * U + u] = bias[half * S + j];
            }
        for (int g = 0; g < 3; ++g) {
            for (int k = 0; k < 2; ++k) out[s.ic + (g * U + u) * 2 + k] = W("I_coarse.weight")[(g * S + j) * 2 + k];
            for (int k = 0; k < 3; ++k) out[s.if_ + (g * U + u) * 3 + k] = W("I_fine.weight")[(g * S + j) * 3 + k];
        }
    }
    for (int r = 0; r < h.dmUO; ++r) {
        const int j = w * h.dmUO + r;
        if (j >= S) continue;
        std::memcpy(out + s.o1 + (size_t)r * S, W("O1.weight") + (size_t)j * S, S * 4);
        std::memcpy(out + s.o3 + (size_t)r * S, W("O3.weight") + (size_t)j * S, S * 4);
        out[s.o1b + r] = W("O1.bias")[j];
        out[s.o3b + r] = W("O3.bias")[j];
    }
    for (int r = 0; r < h.dmUO2; ++r) {
        const int j = w * h.dmUO2 + r;
        if (j >= Q) continue;
        std::memcpy(out + s.o2 + (size_t)r * S, W("O2.weight") + (size_t)j * S, S * 4);
        std::memcpy(out + s.o4 + (size_t)r * S, W("O4.weight") + (size_t)j * S, S * 4);
        out[s.o2b + r] = W("O2.bias")[j];
        out[s.o4b + r] = W("O4.bias")[j];
    }
}

// ---- XCD-resident deepmind kernel (deepmind_xcd.h): the slab of workgroup c (the same on every
// XCD, replicated 8×): A operands [wave][DxA][lane] and constants
static void pack_dx_slab(const wrnn_ctx &h, std::vector<float> &slab) {
    const int H = kDxH, S = kDxS, U = kDxU;
    const DxSlab L = dx_slab_layout();
    slab.assign((size_t)kXcds * kXcdWgs * L.total, 0.0f);
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *R = W("R.weight"), *O1 = W("O1.weight"), *O3 = W("O3.weight"), *O2 = W("O2.weight"), *O4 = W("O4.weight");
    std::vector<float> one((size_t)L.total);
    for (int c = 0; c < kXcdWgs; ++c) {
        std::fill(one.begin(), one.end(), 0.0f);
        // WG-local R row rr = (half·3 + g)·14 + u → R row g·H + half·S + 14c + u
        auto rrow = [&](int rr) {
            const int half = rr / (3 * U), g = (rr / U) % 3, u = rr % U;
            return R + (size_t)(g * H + half * S + U * c + u) * H;
        };
        for (int w = 0; w < kDxWaves; ++w)
            for (int l = 0; l < 64; ++l) {
                const int j = l & 3, b = l >> 2, g4 = b & 3, sp = b >> 2, g2 = b & 1, ks = b >> 1;
                float *A = one.data() + L.a + (size_t)w * kDxA * 64 + l;
                for (int s = 0; s < 5; ++s) {
                    const float *row = rrow(16 * s + 4 * g4 + j);
                    for (int m = 0; m < 56; ++m) {
                        const int col = (m < 28 ? 0 : S) + kDxKW * w + 28 * sp + (m % 28);
                        A[(DA_R + 56 * s + m) * 64] = row[col];
                    }
                }
                {
                    const float *row = rrow(80 + j);
                    for (int m = 0; m < 14; ++m) A[(DA_RQ + m) * 64] = row[(m < 7 ? 0 : S) + kDxKW * w + 7 * b + (m % 7)];
                }
                const int r13 = 4 * g4 + j;
                if (r13 < U)
                    for (int m = 0; m < 28; ++m) {
                        const int col = kDxKW * w + 28 * sp + m;
                        A[(DA_O1 + m) * 64] = O1[(size_t)(U * c + r13) * S + col];
                        A[(DA_O3 + m) * 64] = O3[(size_t)(U * c + r13) * S + col];
                    }
                const int r24 = 4 * g2 + j;
                for (int m = 0; m < 14; ++m) {
                    const int col = kDxKW * w + 14 * ks + m;
                    A[(DA_O2 + m) * 64] = O2[(size_t)(kDxUO2 * c + r24) * S + col];
                    A[(DA_O4 + m) * 64] = O4[(size_t)(kDxUO2 * c + r24) * S + col];
                }
            }
        float *C = one.data() + L.cst;
        for (int r = 0; r < U; ++r) {
            C[DC_B1 + r] = W("O1.bias")[U * c + r];
            C[DC_B3 + r] = W("O3.bias")[U * c + r];
        }
        for (int r = 0; r < kDxUO2; ++r) {
            C[DC_B2 + r] = W("O2.bias")[kDxUO2 * c + r];
            C[DC_B4 + r] = W("O4.bias")[kDxUO2 * c + r];
        }
        for (int g = 0; g < 3; ++g)
            for (int u = 0; u < U; ++u) {
                const int j = U * c + u;
                for (int q = 0; q < 2; ++q) C[DC_IC + (g * U + u) * 2 + q] = W("I_coarse.weight")[(g * S + j) * 2 + q];
                for (int q = 0; q < 3; ++q) C[DC_IF + (g * U + u) * 3 + q] = W("I_fine.weight")[(g * S + j) * 3 + q];
            }
        for (int half = 0; half < 2; ++half)
            for (int u = 0; u < U; ++u) {
                C[DC_BU + half * U + u] = W("bias_u")[half * S + U * c + u];
                C[DC_BR + half * U + u] = W("bias_r")[half * S + U * c + u];
                C[DC_BE + half * U + u] = W("bias_e")[half * S + U * c + u];
            }
        for (int k = 0; k < kXcds; ++k)
            std::copy(one.begin(), one.end(), slab.begin() + (size_t)(k * kXcdWgs + c) * L.total);
    }
}

size_t dm_lds_bytes(const wrnn_ctx &h, int B, int TB) {
    const int S = h.cfg.rnn_dims / 2;
    return (size_t)dm_lds_layout(h.dm_gw ? 0 : h.ds.total, B, TB, S, h.cfg.n_classes, h.dmU, h.G).total * sizeof(float);
}

int dm_tile_for(const wrnn_ctx &h, int B) {
    for (int tb = std::min(B, 16); tb >= 1; --tb)
        if (dm_lds_bytes(h, B, tb) <= (size_t)h.max_lds) return tb;
    return 0;
}

void swap_dm(wrnn_ctx &h, DmPart &p) {
    std::swap(h.ds, p.ds);
    std::swap(h.dmU, p.dmU);
    std::swap(h.dmUO, p.dmUO);
    std::swap(h.dmUO2, p.dmUO2);
    std::swap(h.G, p.G);
    std::swap(h.d_dmslab, p.d_slab);
}


size_t lds_bytes_for(const wrnn_ctx &h, int Bc) {
    return (size_t)lds_layout(h.s.total, Bc, h.cfg.rnn_dims, h.cfg.fc_dims, h.cfg.aux_dims, h.cfg.n_classes, h.NK,
                              h.U, h.UF)
               .total * sizeof(float);
}

// ------------------------------------------------------------- batch-1 role-split kernel
// GRU workgroup g owns units 4g..4g+3 (rows u·3 + gate), FC workgroup f owns fc rows 16f..16f+15
// and the fc3 columns of those rows (fatchord_split.h, slabs).
static void make_split_slabs(wrnn_ctx &h) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, NC = h.cfg.n_classes;
    constexpr int U = kSplitUnits, NF = kSplitFcRows;
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    SplitGruSlab &g = h.sgs;
    g.b3 = take(NC);
    g.wih2 = take(3 * U * R);
    g.whh1 = take(3 * U * R);
    g.whh2 = take(3 * U * R);
    g.q1a = take(3 * R);
    g.q2 = take(3 * U);
    g.wi0 = take(U);
    g.bih1 = take(3 * U);
    g.bhh1 = take(3 * U);
    g.bih2 = take(3 * U);
    g.bhh2 = take(3 * U);
    g.total = o;
    o = 0;
    SplitFcSlab &f = h.sfs;
    f.w3p = take(NF * kSplitLogitLine);
    f.w1 = take(NF * R);
    f.w2 = take(NF * F);
    f.total = o;
}

size_t split_lds_bytes(const wrnn_ctx &h) {
    return (size_t)split_lds_layout(std::max(h.sgs.total, h.sfs.total), h.cfg.rnn_dims, h.cfg.fc_dims).total *
           sizeof(float);
}

static void pack_split_slabs(const wrnn_ctx &h, std::vector<float> &gs, std::vector<float> &fs) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    constexpr int U = kSplitUnits, NF = kSplitFcRows;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    const SplitGruSlab &sg = h.sgs;
    const SplitFcSlab &sf = h.sfs;
    gs.assign((size_t)h.sGg * sg.total, 0.0f);
    fs.assign((size_t)h.sGf * sf.total, 0.0f);
    std::vector<float> q1a(3 * R);
    for (int r = 0; r < 3 * R; ++r) q1a[r] = xcol_dot(W("rnn1.weight_ih_l0") + (size_t)r * R, IW, nin, R);
    for (int w = 0; w < h.sGg; ++w) {
        float *out = gs.data() + (size_t)w * sg.total;
        std::memcpy(out + sg.b3, W("fc3.bias"), (size_t)NC * 4);
        std::memcpy(out + sg.q1a, q1a.data(), (size_t)3 * R * 4);
        for (int u = 0; u < U; ++u) {
            const int j = w * U + u;
            out[sg.wi0 + u] = IW[(size_t)j * nin];
            for (int q = 0; q < 3; ++q) {
                const int src = q * R + j, dst = u * 3 + q;
                const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)src * (R + A);
                std::memcpy(out + sg.wih2 + (size_t)dst * R, ih2, R * 4);
                std::memcpy(out + sg.whh1 + (size_t)dst * R, W("rnn1.weight_hh_l0") + (size_t)src * R, R * 4);
                std::memcpy(out + sg.whh2 + (size_t)dst * R, W("rnn2.weight_hh_l0") + (size_t)src * R, R * 4);
                out[sg.q2 + dst] = xcol_dot(ih2, IW, nin, R);
                out[sg.bih1 + dst] = W("rnn1.bias_ih_l0")[src];
                out[sg.bhh1 + dst] = W("rnn1.bias_hh_l0")[src];
                out[sg.bih2 + dst] = W("rnn2.bias_ih_l0")[src];
                out[sg.bhh2 + dst] = W("rnn2.bias_hh_l0")[src];
            }
        }
    }
    for (int w = 0; w < h.sGf; ++w) {
        float *out = fs.data() + (size_t)w * sf.total;
        for (int e = 0; e < NF; ++e) {
            const int r = w * NF + e;
            for (int j = 0; j < NC; ++j) out[sf.w3p + e * kSplitLogitLine + j] = W("fc3.weight")[(size_t)j * F + r];
            std::memcpy(out + sf.w1 + (size_t)e * R, W("fc1.weight") + (size_t)r * (R + A), R * 4);
            std::memcpy(out + sf.w2 + (size_t)e * F, W("fc2.weight") + (size_t)r * (F + A), F * 4);
        }
    }
}

// Terms-GEMM weights [(Gg + Gf)·kSplitTerms][KX] against X = [cI | a2 a3 a4 | 1 0 0 0]
// (fatchord_split.h, SplitTerm)
static void pack_split_terms_weights(const wrnn_ctx &h, std::vector<float> &Wt) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, KX = h.KX;
    constexpr int U = kSplitUnits, NF = kSplitFcRows;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    Wt.assign((size_t)(h.sGg + h.sGf) * kSplitTerms * KX, 0.0f);
    for (int w = 0; w < h.sGg; ++w)
        for (int u = 0; u < U; ++u) {
            const int j = w * U + u;
            for (int q = 0; q < 3; ++q) {
                const int src = q * R + j;
                float *p1 = Wt.data() + ((size_t)w * kSplitTerms + ST_P1 + u * 3 + q) * KX;
                float *p2 = Wt.data() + ((size_t)w * kSplitTerms + ST_P2 + u * 3 + q) * KX;
                std::memcpy(p1, W("rnn1.weight_ih_l0") + (size_t)src * R, R * 4);
                const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)src * (R + A);
                std::memcpy(p2, ih2, R * 4);
                std::memcpy(p2 + R, ih2 + R, A * 4);                            // a2
            }
            Wt[((size_t)w * kSplitTerms + ST_CI + u) * KX + j] = 1.0f;          // cI_j itself
        }
    for (int f = 0; f < h.sGf; ++f)
        for (int e = 0; e < NF; ++e) {
            const int r = f * NF + e;
            float *v1 = Wt.data() + ((size_t)(h.sGg + f) * kSplitTerms + ST_V1 + e) * KX;
            float *v2 = Wt.data() + ((size_t)(h.sGg + f) * kSplitTerms + ST_V2 + e) * KX;
            std::memcpy(v1 + R + A, W("fc1.weight") + (size_t)r * (R + A) + R, A * 4);   // a3
            v1[R + 3 * A] = W("fc1.bias")[r];
            std::memcpy(v2 + R + 2 * A, W("fc2.weight") + (size_t)r * (F + A) + F, A * 4);   // a4
            v2[R + 3 * A] = W("fc2.bias")[r];
        }
}

// ---- XCD-resident kernel (fatchord_xcd.h): workgroup c of an XCD owns units and fc rows
// 16c..16c+15; wave w of it units / fc rows 16c + 2w + {0, 1}
static void make_xcd_slab(wrnn_ctx &h) {
    const int R = h.cfg.rnn_dims;
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    XcdSlab &x = h.xs;
    x.wih2 = take(kXWaves * 6 * R);
    x.w1 = take(kXWaves * 2 * R);
    x.w2 = take(kXWaves * 2 * R);
    x.whh2 = take(48 * R);
    x.whh1 = take(48 * R);
    x.w3 = take(kXWaves * 2 * 32);
    x.q1a = take(3 * R);
    x.cst = take(kXCst);
    x.total = o;
}

static void pack_xcd_slab(const wrnn_ctx &h, std::vector<float> &slab) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    const XcdSlab &x = h.xs;
    slab.assign((size_t)kXcdWgs * x.total, 0.0f);
    std::vector<float> q1a(3 * R);
    for (int r = 0; r < 3 * R; ++r) q1a[r] = xcol_dot(W("rnn1.weight_ih_l0") + (size_t)r * R, IW, nin, R);
    for (int c = 0; c < kXcdWgs; ++c) {
        float *out = slab.data() + (size_t)c * x.total;
        std::memcpy(out + x.q1a, q1a.data(), (size_t)3 * R * 4);
        for (int w = 0; w < kXWaves; ++w)   // unit pairs (fatchord_xcd.h: GRU2 group g takes pairs 2g, 2g + 1)
            for (int i = 0; i < 2; ++i) {
                const int u = 2 * w + i, j = c * kXUnits + u;     // unit j, fc row j
                for (int q = 0; q < 3; ++q)
                    std::memcpy(out + x.wih2 + (size_t)(w * 6 + 2 * q + i) * R,
                                W("rnn2.weight_ih_l0") + (size_t)(q * R + j) * (R + A), R * 4);
                std::memcpy(out + x.w1 + (size_t)(w * 2 + i) * R, W("fc1.weight") + (size_t)j * (R + A), R * 4);
                std::memcpy(out + x.w2 + (size_t)(w * 2 + i) * R, W("fc2.weight") + (size_t)j * (F + A), F * 4);
                for (int k = 0; k < NC; ++k) out[x.w3 + (w * 2 + i) * 32 + k] = W("fc3.weight")[(size_t)k * F + j];
            }
        for (int u = 0; u < kXUnits; ++u) {
            const int j = c * kXUnits + u;
            out[x.cst + XC_WI0 + u] = IW[(size_t)j * nin];
            for (int q = 0; q < 3; ++q) {
                const int src = q * R + j, rr = u * 3 + q;
                std::memcpy(out + x.whh1 + (size_t)rr * R, W("rnn1.weight_hh_l0") + (size_t)src * R, R * 4);
                std::memcpy(out + x.whh2 + (size_t)rr * R, W("rnn2.weight_hh_l0") + (size_t)src * R, R * 4);
                out[x.cst + XC_Q2 + rr] = xcol_dot(W("rnn2.weight_ih_l0") + (size_t)src * (R + A), IW, nin, R);
                out[x.cst + XC_BIH1 + rr] = W("rnn1.bias_ih_l0")[src];
                out[x.cst + XC_BHH1 + rr] = W("rnn1.bias_hh_l0")[src];
                out[x.cst + XC_BIH2 + rr] = W("rnn2.bias_ih_l0")[src];
                out[x.cst + XC_BHH2 + rr] = W("rnn2.bias_hh_l0")[src];
            }
        }
        for (int k = 0; k < NC; ++k) out[x.cst + XC_B3 + k] = W("fc3.bias")[k];
    }
}

// The XCD kernels' terms-GEMM rows against X' = [mel | a1 | a2 | a3 | a4 | 1 0 0 0] (KXc = CD + 4):
// the I layer (fatchord_version.py:208, cI = W_I·[mel; a1] + b_I; the x column is folded
// separately, q1a / q2) is composed into the W_ih1 / W_ih2 rows in fp64 here, so the GEMM runs on
// the 208-wide conditioning record instead of a 900-wide cI (4.7x less work at rnn 896).
static void fold_ci_row(const wrnn_ctx &h, const float *w, float *dst) {
    const int R = h.cfg.rnn_dims, M = h.cfg.feat_dims, A = h.cfg.aux_dims, nin = 1 + M + A;
    const float *IW = h.w.at("I.weight").data(), *Ib = h.w.at("I.bias").data();
    std::vector<double> acc(M + A + 1, 0.0);
    for (int k = 0; k < R; ++k) {
        const double wk = w[k];
        if (wk == 0.0) continue;
        const float *iw = IW + (size_t)k * nin + 1;
        for (int m = 0; m < M + A; ++m) acc[m] += wk * iw[m];
        acc[M + A] += wk * Ib[k];
    }
    for (int m = 0; m < M + A; ++m) dst[m] += (float)acc[m];
    dst[h.CD] += (float)acc[M + A];
}

// slot rows of one unit j (gates q = 0..2: p1q[q], p2q[q]; its cI: ci) and of one fc row r
// (v1, v2) for the composed input X'
static void pack_xcd_unit_terms(const wrnn_ctx &h, int j, float *const p1q[3], float *const p2q[3], float *ci) {
    const int R = h.cfg.rnn_dims, M = h.cfg.feat_dims, A = h.cfg.aux_dims, nin = 1 + M + A;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    for (int q = 0; q < 3; ++q) {
        const int src = q * R + j;
        fold_ci_row(h, W("rnn1.weight_ih_l0") + (size_t)src * R, p1q[q]);
        const float *ih2 = W("rnn2.weight_ih_l0") + (size_t)src * (R + A);
        fold_ci_row(h, ih2, p2q[q]);
        for (int a = 0; a < A; ++a) p2q[q][M + A + a] += ih2[R + a];                      // a2
    }
    const float *iw = W("I.weight") + (size_t)j * nin + 1;
    for (int m = 0; m < M + A; ++m) ci[m] = iw[m];                                         // cI_j
    ci[h.CD] = W("I.bias")[j];
}
static void pack_xcd_fc_terms(const wrnn_ctx &h, int r, float *v1, float *v2) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, M = h.cfg.feat_dims, A = h.cfg.aux_dims;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    for (int a = 0; a < A; ++a) {
        v1[M + 2 * A + a] = W("fc1.weight")[(size_t)r * (R + A) + R + a];                 // a3
        v2[M + 3 * A + a] = W("fc2.weight")[(size_t)r * (F + A) + F + a];                 // a4
    }
    v1[h.CD] = W("fc1.bias")[r];
    v2[h.CD] = W("fc2.bias")[r];
}

// Terms-GEMM weights [kXcdWgs·kXTerms][KXc] (XTerm slots) against X'
static void pack_xcd_terms_weights(const wrnn_ctx &h, std::vector<float> &Wt) {
    const int KX = h.KXc;
    Wt.assign((size_t)kXcdWgs * kXTerms * KX, 0.0f);
    for (int c = 0; c < kXcdWgs; ++c) {
        auto row = [&](int slot) { return Wt.data() + ((size_t)c * kXTerms + slot) * KX; };
        for (int u = 0; u < kXUnits; ++u) {
            float *const p1q[3] = {row(XT_P1 + u * 3), row(XT_P1 + u * 3 + 1), row(XT_P1 + u * 3 + 2)};
            float *const p2q[3] = {row(XT_P2 + u * 3), row(XT_P2 + u * 3 + 1), row(XT_P2 + u * 3 + 2)};
            pack_xcd_unit_terms(h, c * kXUnits + u, p1q, p2q, row(XT_CI + u));
            pack_xcd_fc_terms(h, c * kXUnits + u, row(XT_V1 + u), row(XT_V2 + u));
        }
    }
}

// Many-row kernel: its compact terms record (kMRing slots per workgroup, MT_ order) segmented by
// GEMM group (fatchord_xcdm.h, mterm_off) with the columns in the split input order X'' = [mel |
// a1 | 1 | a2 | a3 | a4 | 1 | 0 0] (pack_cond_input_kernel, split = M + A): P1 and cI depend on
// mel‖a1 and their bias only, P2 also on a2, V1 / V2 on a3 / a4 and their biases — generate_xcdm
// runs one GEMM per group over just those columns (xcdm_terms_gemms).
static void pack_xcdm_terms_weights(const wrnn_ctx &h, std::vector<float> &Wm) {
    std::vector<float> Wt;
    pack_xcd_terms_weights(h, Wt);
    const int KX = h.KXc, CD = h.CD, split = h.cfg.feat_dims + h.cfg.aux_dims;
    Wm.assign((size_t)kXcdWgs * kMRing * KX, 0.0f);
    for (int c = 0; c < kXcdWgs; ++c)
        for (int s = 0; s < kMRing; ++s) {
            const float *src = Wt.data() + ((size_t)c * kXTerms + mterm_xt(s)) * KX;
            float *dst = Wm.data() + (size_t)mterm_off(c, s) * KX;
            for (int j = 0; j < CD; ++j) dst[j < split ? j : j + 1] = src[j];
            dst[s >= MT_V1 ? CD + 1 : split] = src[CD];          // the bias → its group's ones column
        }
}

// (record rows, first input column, depth) of each group: [P1 | cI] on mel‖a1‖1, P2 on
// mel‖a1‖1‖a2, [V1 | V2] on a3‖a4‖1 — depths rounded up to a multiple of 4 over zero weights
void xcdm_terms_gemms(const wrnn_ctx &h, XcdmGemm (&g)[3]) {
    const int M = h.cfg.feat_dims, A = h.cfg.aux_dims, split = M + A;
    auto up4 = [](int n) { return (n + 3) / 4 * 4; };
    const int v0 = (split + 1 + A) / 4 * 4;                     // first column of a3, rounded down
    g[0] = {kMG0, kMG1 - kMG0, 0, std::min(up4(split + 1), h.KXc)};
    g[1] = {kMG1, kMG2 - kMG1, 0, std::min(up4(split + 1 + A), h.KXc)};
    g[2] = {kMG2, kMGEnd - kMG2, v0, std::min(up4(h.CD + 2 - v0), h.KXc - v0)};
}

// ---- XCD-resident block-sparse kernel (fatchord_xcds.h): workgroup c of an XCD owns units
// 28c..28c+27 (block-rows ub = 0..6 of each gate) and fc rows 16c..16c+15
static void make_xcds_slab(wrnn_ctx &h) {
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    XcdsSlab &x = h.xss;
    x.wih2b = take(kSBR * kSNB * 16);
    x.whh1b = take(kSBR * kSNB * 16);
    x.whh2b = take(kSBR * kSNB * 16);
    x.wih2c = take(kSBR * kSNB);
    x.whh1c = take(kSBR * kSNB);
    x.whh2c = take(kSBR * kSNB);
    x.w1 = take(kXFcRows * kSR);
    x.w2 = take(kXFcRows * 512);
    x.w3 = take(kXFcRows * 32);
    x.q1a = take(3 * kSR);
    x.cst = take(kSCst);
    x.total = o;
}

// nonzero 4x4 blocks of the gate block-row (q, 4-unit group u4) of a loop matrix
static std::vector<int> xcds_blocks(const LoopMat &m, int q, int u4) {
    std::vector<int> cols;
    for (int cb = 0; cb < kSR; cb += 4)
        if (block_nonzero(m.w, m.ld, q * kSR + 4 * u4, cb)) cols.push_back(cb / 4);
    return cols;
}

// largest nonzero-block count over every gate block-row of W_ih2[:, :R], W_hh1, W_hh2
static int xcds_nbmax(const wrnn_ctx &h) {
    LoopMat m[3];
    loop_mats(h, m);
    int mx = 0;
    for (int k = 0; k < 3; ++k)
        for (int q = 0; q < 3; ++q)
            for (int u4 = 0; u4 < kSR / 4; ++u4) mx = std::max(mx, (int)xcds_blocks(m[k], q, u4).size());
    return mx;
}

static void pack_xcds_slab(const wrnn_ctx &h, std::vector<float> &slab) {
    const int R = kSR, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    const XcdsSlab &x = h.xss;
    slab.assign((size_t)kXcdWgs * x.total, 0.0f);
    std::vector<float> q1a(3 * R);
    for (int r = 0; r < 3 * R; ++r) q1a[r] = xcol_dot(W("rnn1.weight_ih_l0") + (size_t)r * R, IW, nin, R);
    LoopMat m[3];
    loop_mats(h, m);
    const int boff[3] = {x.wih2b, x.whh1b, x.whh2b}, coff[3] = {x.wih2c, x.whh1c, x.whh2c};
    for (int c = 0; c < kXcdWgs; ++c) {
        float *out = slab.data() + (size_t)c * x.total;
        std::memcpy(out + x.q1a, q1a.data(), (size_t)3 * R * 4);
        for (int k = 0; k < 3; ++k)
            for (int q = 0; q < 3; ++q)
                for (int ub = 0; ub < kSUB; ++ub) {
                    const int br = q * kSUB + ub, u4 = c * kSUB + ub, r0 = q * R + 4 * u4;
                    const std::vector<int> cols = xcds_blocks(m[k], q, u4);
                    int *cc = reinterpret_cast<int *>(out + coff[k]) + br * kSNB;
                    for (size_t n = 0; n < cols.size() && n < (size_t)kSNB; ++n) {
                        float *blk = out + boff[k] + ((size_t)br * kSNB + n) * 16;
                        for (int r = 0; r < 4; ++r)
                            for (int cc4 = 0; cc4 < 4; ++cc4)
                                blk[r * 4 + cc4] = m[k].w[(size_t)(r0 + r) * m[k].ld + 4 * cols[n] + cc4];
                        cc[n] = cols[n];
                    }
                }
        for (int r = 0; r < kXFcRows; ++r) {
            const int j = c * kXFcRows + r;
            std::memcpy(out + x.w1 + (size_t)r * R, W("fc1.weight") + (size_t)j * (R + A), R * 4);
            std::memcpy(out + x.w2 + (size_t)r * F, W("fc2.weight") + (size_t)j * (F + A), F * 4);
            for (int kk = 0; kk < NC; ++kk) out[x.w3 + r * 32 + kk] = W("fc3.weight")[(size_t)kk * F + j];
        }
        for (int u = 0; u < kSU; ++u) {
            const int j = c * kSU + u;
            out[x.cst + SC_WI0 + u] = IW[(size_t)j * nin];
            for (int q = 0; q < 3; ++q) {
                const int src = q * R + j, rr = u * 3 + q;
                out[x.cst + SC_Q2 + rr] = xcol_dot(W("rnn2.weight_ih_l0") + (size_t)src * (R + A), IW, nin, R);
                out[x.cst + SC_BIH1 + rr] = W("rnn1.bias_ih_l0")[src];
                out[x.cst + SC_BHH1 + rr] = W("rnn1.bias_hh_l0")[src];
                out[x.cst + SC_BIH2 + rr] = W("rnn2.bias_ih_l0")[src];
                out[x.cst + SC_BHH2 + rr] = W("rnn2.bias_hh_l0")[src];
            }
        }
        for (int kk = 0; kk < NC; ++kk) out[x.cst + SC_B3 + kk] = W("fc3.bias")[kk];
    }
}

// Terms-GEMM weights [kXcdWgs·kSTerms][KXc] (SXTerm slots) against X' (pack_xcd_terms_weights)
static void pack_xcds_terms_weights(const wrnn_ctx &h, std::vector<float> &Wt) {
    const int KX = h.KXc;
    Wt.assign((size_t)kXcdWgs * kSTerms * KX, 0.0f);
    for (int c = 0; c < kXcdWgs; ++c) {
        auto row = [&](int slot) { return Wt.data() + ((size_t)c * kSTerms + slot) * KX; };
        for (int u = 0; u < kSU; ++u) {
            float *const p1q[3] = {row(SX_P1 + u * 3), row(SX_P1 + u * 3 + 1), row(SX_P1 + u * 3 + 2)};
            float *const p2q[3] = {row(SX_P2 + u * 3), row(SX_P2 + u * 3 + 1), row(SX_P2 + u * 3 + 2)};
            pack_xcd_unit_terms(h, c * kSU + u, p1q, p2q, row(SX_CI + u));
        }
        for (int r = 0; r < kXFcRows; ++r) pack_xcd_fc_terms(h, c * kXFcRows + r, row(SX_V1 + r), row(SX_V2 + r));
    }
}

// ---- XCD-resident many-row kernel (fatchord_xcdm.h): per workgroup c the MFMA A operands of the
// eleven 16-row sets (wave w: K window [kMK·w, kMK·(w + 1))), the fc3 columns of its f2 rows and
// the small vectors
static void make_xcdm_slab(wrnn_ctx &h) {
    int o = 0;
    auto take = [&](int n) { int at = o; o += round4(n); return at; };
    XcdmSlab &x = h.xms;
    const bool raw = h.cfg.mode == WRNN_MODE_RAW;
    x.a = take(kMWaves * kMSets * kMJ * 64);
    x.a3 = take(raw ? kMWaves * kMJ * 64 : 0);
    x.w3 = take(raw ? 0 : 32 * kMW3Stride);
    x.cst = take(kMCst);
    x.total = o;
}

static void pack_xcdm_slab(const wrnn_ctx &h, std::vector<float> &slab) {
    const int R = h.cfg.rnn_dims, F = h.cfg.fc_dims, A = h.cfg.aux_dims, NC = h.cfg.n_classes;
    auto W = [&](const char *n) { return h.w.at(n).data(); };
    const float *IW = W("I.weight");
    const int nin = 1 + h.cfg.feat_dims + A;
    const XcdmSlab &x = h.xms;
    slab.assign((size_t)kXcdWgs * x.total, 0.0f);
    // row r (0..15) of set s of workgroup c: (matrix, row index, row stride)
    auto set_row = [&](int s, int c, int r) -> const float * {
        if (s < MS_FC1) return W("rnn2.weight_ih_l0") + (size_t)(s * R + 16 * c + r) * (R + A);
        if (s == MS_FC1) return W("fc1.weight") + (size_t)(16 * c + r) * (R + A);
        if (s == MS_FC2) return W("fc2.weight") + (size_t)(16 * c + r) * (F + A);
        if (s < MS_HH1) return W("rnn2.weight_hh_l0") + (size_t)((s - MS_HH2) * R + 16 * c + r) * R;
        return W("rnn1.weight_hh_l0") + (size_t)((s - MS_HH1) * R + 16 * c + r) * R;
    };
    for (int c = 0; c < kXcdWgs; ++c) {
        float *out = slab.data() + (size_t)c * x.total;
        for (int w = 0; w < kMWaves; ++w)
            for (int s = 0; s < kMSets; ++s)
                for (int j = 0; j < kMJ; ++j)
                    for (int l = 0; l < 64; ++l) {
                        const int g = (l >> 2) & 3, sp = l >> 4, j4 = l & 3;
                        out[x.a + (((size_t)w * kMSets + s) * kMJ + j) * 64 + l] =
                            set_row(s, c, 4 * g + j4)[kMK * w + kMJ * sp + j];
                    }
        if (h.cfg.mode == WRNN_MODE_RAW) {   // fc3 rows of the own classes 16c + r, [wave][k-chunk][lane][4]
            for (int w = 0; w < kMWaves; ++w)
                for (int j = 0; j < kMJ; ++j)
                    for (int l = 0; l < 64; ++l)
                        out[x.a3 + ((size_t)(w * (kMJ / 4) + j / 4) * 64 + l) * 4 + (j & 3)] =
                            W("fc3.weight")[(size_t)(16 * c + (l & 15)) * F + kMK * w + kMJ * (l >> 4) + j];
        } else {
            for (int jj = 0; jj < NC; ++jj)
                for (int r = 0; r < 16; ++r) out[x.w3 + jj * kMW3Stride + r] = W("fc3.weight")[(size_t)jj * F + 16 * c + r];
        }
        for (int u = 0; u < 16; ++u) {
            const int j = 16 * c + u;
            out[x.cst + MC_WI0 + u] = IW[(size_t)j * nin];
            for (int q = 0; q < 3; ++q) {
                const int src = q * R + j, i = q * 16 + u;
                out[x.cst + MC_Q1 + i] = xcol_dot(W("rnn1.weight_ih_l0") + (size_t)src * R, IW, nin, R);
                out[x.cst + MC_Q2 + i] = xcol_dot(W("rnn2.weight_ih_l0") + (size_t)src * (R + A), IW, nin, R);
                out[x.cst + MC_BIH1 + i] = W("rnn1.bias_ih_l0")[src];
                out[x.cst + MC_BHH1 + i] = W("rnn1.bias_hh_l0")[src];
                out[x.cst + MC_BIH2 + i] = W("rnn2.bias_ih_l0")[src];
                out[x.cst + MC_BHH2 + i] = W("rnn2.bias_hh_l0")[src];
            }
        }
        if (h.cfg.mode == WRNN_MODE_RAW)
            for (int r = 0; r < 16; ++r) out[x.cst + MC_B3 + r] = W("fc3.bias")[16 * c + r];
        else
            for (int jj = 0; jj < NC; ++jj) out[x.cst + MC_B3 + jj] = W("fc3.bias")[jj];
    }
}

}  // namespace host
}  // namespace wrnn

int wrnn_create(const wrnn_config *cfg, int device, wrnn_t **out) {
    if (!out || !cfg) return WRNN_EINVAL;
    *out = nullptr;
    if (cfg->abi_version != WRNN_ABI_VERSION) return WRNN_EINVAL;
    auto *h = new (std::nothrow) wrnn_ctx();
    if (!h) return WRNN_ENOMEM;
    *out = h;
    h->cfg = *cfg;
    h->device = device;
    const wrnn_config &c = h->cfg;
    const bool mol = c.mode == WRNN_MODE_MOL;
    if (c.mode != WRNN_MODE_MOL && c.mode != WRNN_MODE_RAW && c.mode != WRNN_MODE_DM)
        return fail(h, WRNN_EINVAL, "unknown mode");
    if (c.rnn_dims <= 0 || c.n_classes <= 0 ||
        (c.mode != WRNN_MODE_DM && (c.fc_dims <= 0 || c.aux_dims <= 0 || c.feat_dims <= 0)))
        return fail(h, WRNN_EINVAL, "dims must be positive");
    if (c.mode != WRNN_MODE_DM && (c.rnn_dims % 4 || c.fc_dims % 4 || c.aux_dims % 4))
        return fail(h, WRNN_EUNSUPPORTED, "rnn_dims, fc_dims and aux_dims must be multiples of 4");
    if (mol && c.n_classes != 30) return fail(h, WRNN_EINVAL, "MOL mode has n_classes = 30 (10 logistics)");
    HIP_TRY(h, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(h, hipGetDeviceProperties(&prop, device));
    h->num_cus = prop.multiProcessorCount;
    h->max_lds = std::max<int>((int)prop.sharedMemPerBlock, (int)prop.maxSharedMemoryPerMultiProcessor);
    h->max_lds = std::min(h->max_lds, 160 * 1024);
    if (c.mode == WRNN_MODE_DM) {   // deepmind_version: the multi-row dual-softmax kernel only
        const int H = c.rnn_dims, S = H / 2, Q = c.n_classes;
        if (S % 4) return fail(h, WRNN_EUNSUPPORTED, "DM hidden_size must be a multiple of 8");
        const int gt = c.grid > 0 ? c.grid : h->num_cus;
        h->dm = true;
        h->dmU = (S + gt - 1) / gt;
        h->G = (S + h->dmU - 1) / h->dmU;
        h->dmUO = (S + h->G - 1) / h->G;
        h->dmUO2 = (Q + h->G - 1) / h->G;
        h->KA = round4(std::max(S, Q));
        h->NK = 2 * Q;
        h->ds = make_dm_slab(*h);
        if (dm_tile_for(*h, 1) == 0) h->dm_gw = true;   // weights beyond LDS: stream the slab
        if (dm_tile_for(*h, 1) == 0)
            return fail(h, WRNN_EUNSUPPORTED, "DM: one row of state does not fit LDS (" + std::to_string(dm_lds_bytes(*h, 1, 1)) + " B)");
        HIP_TRY(h, prepare_dm_kernel(h->max_lds));
        int per_cu = 0;
        HIP_TRY(h, dm_occupancy(&per_cu, dm_lds_bytes(*h, 1, 1)));
        if (per_cu * h->num_cus < h->G)
            return fail(h, WRNN_EUNSUPPORTED, "DM persistent grid is not co-resident");
        // two row groups of G/2 workgroups (twice the units each), as the fatchord rows kernel
        if (h->G % 2 == 0 && h->G >= 8 && !h->dm_gw) {
            DmPart p{};
            p.G = h->G / 2;
            p.dmU = (S + p.G - 1) / p.G;
            p.G = (S + p.dmU - 1) / p.dmU;
            p.dmUO = (S + p.G - 1) / p.G;
            p.dmUO2 = (Q + p.G - 1) / p.G;
            h->dm2 = p;
            bool ok = false;
            {
                DmScope sc(*h, h->dm2, true);
                h->ds = make_dm_slab(*h);
                if (dm_tile_for(*h, 2) > 0) {
                    HIP_TRY(h, dm_occupancy(&per_cu, dm_lds_bytes(*h, 1, 1)));
                    ok = per_cu * h->num_cus >= 2 * h->G;
                }
            }
            h->dm2.ok = ok;
        }
        // hidden 896 / quantisation 256 on a full 8 × 32-CU MI355X: the XCD-resident MFMA kernel
        if (H == kDxH && Q == kDxQ && c.grid <= 0 && h->num_cus == kXcds * kXcdWgs) {
            bool ok = false;
            HIP_TRY(h, prepare_dx_kernel(h->max_lds, &ok));
            h->dx_ok = ok;
        }
        h->timeout_ticks = (long long)(c.timeout_ms > 0 ? c.timeout_ms : 2000) * 100000LL;
        HIP_TRY(h, hipMalloc(&h->d_ctl, kCtlWords * sizeof(int)));
        HIP_TRY(h, hipMemset(h->d_ctl, 0, kCtlWords * sizeof(int)));
        HIP_TRY(h, hipEventCreate(&h->ev0));
        HIP_TRY(h, hipEventCreate(&h->ev1));
        return WRNN_OK;
    }
    const int R = c.rnn_dims, F = c.fc_dims;
    const int gtarget = c.grid > 0 ? c.grid : h->num_cus;
    h->U = (R + gtarget - 1) / gtarget;
    h->G = (R + h->U - 1) / h->U;
    h->UF = (F + h->G - 1) / h->G;
    h->UC = mol ? 0 : (c.n_classes + h->G - 1) / h->G;
    h->NMAX = std::max(R, std::max(F, c.n_classes));
    h->NK = mol ? 11 : c.n_classes;
    h->CD = c.feat_dims + 4 * c.aux_dims;
    h->s = make_slab_layout(*h);
    // rows per launch: LDS, and the per-thread gather register budget
    h->KX = R + 3 * c.aux_dims + 4;
    h->KXc = h->CD + 4;
    h->KA = round4(std::max(R, std::max(F, c.n_classes)));
    set_rows_partition(*h, 0);
    // dims whose dense weights fit neither kernel may still run with block-sparse GRU weights
    // (decided at wrnn_set_weights)
    const bool sparse_possible = R % 4 == 0 && R / 4 <= h->num_cus;
    h->max_rows = 0;
    for (int b = 1; b <= 64; ++b) {
        if (lds_bytes_for(*h, b) > (size_t)h->max_lds) break;
        // one polling wave: kGatherMax slots per lane in the generic kernels, exact counts (rows ≤ 2)
        // in the compile-time-dims ones
        const bool fast = loop_has_fast_path(R, F, c.aux_dims, c.n_classes, mol, h->U, h->UF, h->UC);
        if (fast ? b > 2 : (size_t)b * h->NMAX > (size_t)kPollThreads * kGatherMax) break;
        h->max_rows = b;
    }
    if (h->max_rows < 1 && !h->rows_ok && !sparse_possible)
        return fail(h, WRNN_EUNSUPPORTED, "weight slab + one row of state exceeds LDS (" +
                                              std::to_string(lds_bytes_for(*h, 1)) + " B)");
    HIP_TRY(h, prepare_loop_kernel(h->max_lds));
    HIP_TRY(h, prepare_rows_kernel(h->max_lds));
    int per_cu = 0;
    if (h->max_rows >= 1) {
        HIP_TRY(h, loop_occupancy(&per_cu, lds_bytes_for(*h, h->max_rows)));
        if (per_cu * h->num_cus < h->G)
            return fail(h, WRNN_EUNSUPPORTED, "persistent grid of " + std::to_string(h->G) +
                                                  " workgroups is not co-resident (" + std::to_string(per_cu) +
                                                  "/CU × " + std::to_string(h->num_cus) + " CUs)");
    }
    if (h->rows_ok) {
        HIP_TRY(h, rows_occupancy(&per_cu, rows_lds_bytes(*h, 1, 1)));
        if (per_cu * h->num_cus < h->rG) h->rows_ok = false;
    }
    set_group_partition(*h);
    if (h->g2.ok) {
        PartScope ps(*h, h->g2, true);
        // the partition is accepted on its fit with the MoL head left in HBM (set_group_partition); where
        // the head does not fit beside the body a launch leaves it there, so residency is asked for that
        // size (with the head counted, occupancy was 0 and such a model silently kept one group)
        const bool head = rows_tile_for(*h, 1) > 0;
        HIP_TRY(h, rows_occupancy(&per_cu, rows_lds_bytes(*h, 1, 1, head)));
        if (per_cu * h->num_cus < 2 * h->rG) h->rows_ok = false;
    }
    // one MoL row: the role-split kernel (compile-time dims) when its grid and LDS fit; an
    // explicit grid request keeps the uniform kernels
    if (mol && c.grid <= 0 && split_has_kernel(R, F) && R % kSplitUnits == 0 && F % kSplitFcRows == 0) {
        h->sGg = R / kSplitUnits;
        h->sGf = F / kSplitFcRows;
        make_split_slabs(*h);
        if (h->sGg + h->sGf <= h->num_cus && split_lds_bytes(*h) <= (size_t)h->max_lds) {
            HIP_TRY(h, prepare_split_kernel(h->max_lds));
            HIP_TRY(h, split_occupancy(&per_cu, split_lds_bytes(*h)));
            h->split_ok = per_cu >= 1;
        }
    }
    // MoL rnn / fc 512: the XCD-resident kernel (one row per XCD) on a full 8 × 32-CU MI355X
    if (mol && c.grid <= 0 && R == 512 && F == 512 && c.aux_dims == 32 && h->num_cus == kXcds * kXcdWgs &&
        xcd_lds_layout().total * sizeof(float) <= (size_t)h->max_lds) {
        make_xcd_slab(*h);
        HIP_TRY(h, prepare_xcd_kernel(h->max_lds));
        HIP_TRY(h, xcd_occupancy(&per_cu));
        h->xcd_ok = per_cu >= 1;
        // its many-row form (same terms GEMM)
        if (h->xcd_ok) {
            make_xcdm_slab(*h);
            HIP_TRY(h, prepare_xcdm_kernel(h->max_lds));
            HIP_TRY(h, xcdm_max_quads(h->max_lds, false, &h->xcdm_nq));
            h->xcdm_ok = h->xcdm_nq >= 1;
            if (h->xcdm_nq >= kMQuadMax) HIP_TRY(h, prepare_xcdm_group_kernel(h->max_lds, false, &h->xcdmg_ok));
        }
    }
    // RAW 9-bit, rnn / fc 512: the many-row XCD-resident kernel with the softmax head (every row count)
    if (!mol && c.grid <= 0 && R == 512 && F == 512 && c.aux_dims == 32 && c.n_classes == kMRawNC &&
        h->num_cus == kXcds * kXcdWgs) {
        make_xcdm_slab(*h);
        HIP_TRY(h, prepare_xcdm_kernel(h->max_lds));
        HIP_TRY(h, xcdm_max_quads(h->max_lds, true, &h->xcdm_nq));
        h->xcdm_ok = h->xcdm_nq >= 1;
        if (h->xcdm_nq >= kMQuadMax) HIP_TRY(h, prepare_xcdm_group_kernel(h->max_lds, true, &h->xcdmg_ok));
    }
    // MoL rnn 896 / fc 512: the XCD-resident block-sparse kernel, if the weights turn out
    // block-sparse (decided at wrnn_set_weights)
    if (mol && c.grid <= 0 && R == kSR && F == 512 && c.aux_dims == 32 && h->num_cus == kXcds * kXcdWgs &&
        xcds_lds_layout().total * sizeof(float) <= (size_t)h->max_lds) {
        make_xcds_slab(*h);
        HIP_TRY(h, prepare_xcds_kernel(h->max_lds));
        HIP_TRY(h, xcds_occupancy(&per_cu));
        h->xcds_cap = per_cu >= 1;
    }
    h->timeout_ticks = (long long)(c.timeout_ms > 0 ? c.timeout_ms : 2000) * 100000LL;   // 100 MHz
    HIP_TRY(h, hipMalloc(&h->d_ctl, kCtlWords * sizeof(int)));
    HIP_TRY(h, hipMemset(h->d_ctl, 0, kCtlWords * sizeof(int)));
    HIP_TRY(h, hipEventCreate(&h->ev0));
    HIP_TRY(h, hipEventCreate(&h->ev1));
    return WRNN_OK;
}

int wrnn_set_weights(wrnn_t *h, const wrnn_tensor *tensors, int n) {
    if (!h || (n > 0 && !tensors)) return WRNN_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    const auto need = required(h->cfg);
    // whatever follows, the slabs no longer hold the weights an open session started with
    if (n > 0) ++h->loads;
    for (int i = 0; i < n; ++i) {
        const wrnn_tensor &t = tensors[i];
        if (!t.name || !t.data) return fail(h, WRNN_EINVAL, "null tensor name/data");
        auto it = std::find_if(need.begin(), need.end(), [&](const Need &q) { return t.name == std::string(q.name); });
        if (it == need.end()) continue;   // load_state_dict(strict=False): ignore others
        if (t.numel != it->rows * it->cols)
            return fail(h, WRNN_EINVAL, std::string(t.name) + ": expected " + std::to_string(it->rows * it->cols) +
                                            " elements, got " + std::to_string(t.numel));
        std::vector<float> v((size_t)t.numel);
        if (t.on_device)
            HIP_TRY(h, hipMemcpy(v.data(), t.data, (size_t)t.numel * 4, hipMemcpyDeviceToHost));
        else
            std::memcpy(v.data(), t.data, (size_t)t.numel * 4);
        h->w[t.name] = std::move(v);
    }
    for (const auto &q : need)
        if (!h->w.count(q.name)) { h->ready = false; return WRNN_OK; }   // partial load so far
    if (h->dm) {
        for (int grouped = 0; grouped < (h->dm2.ok ? 2 : 1); ++grouped) {
            DmScope sc(*h, h->dm2, grouped == 1);
            std::vector<float> slab((size_t)h->G * h->ds.total);
            for (int w = 0; w < h->G; ++w) pack_dm_slab(*h, w, slab.data() + (size_t)w * h->ds.total);
            if (h->d_dmslab) HIP_TRY(h, hipFree(h->d_dmslab));
            h->d_dmslab = nullptr;
            HIP_TRY(h, hipMalloc(&h->d_dmslab, slab.size() * 4));
            HIP_TRY(h, hipMemcpy(h->d_dmslab, slab.data(), slab.size() * 4, hipMemcpyHostToDevice));
        }
        if (h->dx_ok) {
            std::vector<float> slab;
            pack_dx_slab(*h, slab);
            if (h->d_dxslab) HIP_TRY(h, hipFree(h->d_dxslab));
            h->d_dxslab = nullptr;
            HIP_TRY(h, hipMalloc(&h->d_dxslab, slab.size() * 4));
            HIP_TRY(h, hipMemcpy(h->d_dxslab, slab.data(), slab.size() * 4, hipMemcpyHostToDevice));
        }
        h->ready = true;
        return WRNN_OK;
    }
    // pack and upload
    if (h->max_rows >= 1) {
        std::vector<float> slab((size_t)h->G * h->s.total);
        for (int w = 0; w < h->G; ++w) pack_slab(*h, w, slab.data() + (size_t)w * h->s.total);
        if (!h->d_slab) HIP_TRY(h, hipMalloc(&h->d_slab, slab.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_slab, slab.data(), slab.size() * 4, hipMemcpyHostToDevice));
    }
    const auto &IW = h->w.at("I.weight");
    const auto &Ib = h->w.at("I.bias");
    if (!h->d_IW) HIP_TRY(h, hipMalloc(&h->d_IW, IW.size() * 4));
    if (!h->d_Ib) HIP_TRY(h, hipMalloc(&h->d_Ib, Ib.size() * 4));
    HIP_TRY(h, hipMemcpy(h->d_IW, IW.data(), IW.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_Ib, Ib.data(), Ib.size() * 4, hipMemcpyHostToDevice));
    // rows kernel: block-sparse GRU weights (pruning.py) are kept as nonzero 4x4 blocks when the
    // block density is <= 1/2 (WRNN_SPARSE=0 keeps them dense)
    {
        const int R = h->cfg.rnn_dims;
        int nbmax = 0;
        double density = 1.0;
        const char *sp_env = std::getenv("WRNN_SPARSE");
        if (R % 4 == 0 && R / 4 <= h->num_cus && !(sp_env && std::string(sp_env) == "0"))
            block_stats(*h, &nbmax, &density);
        set_rows_partition(*h, density <= 0.5 ? std::max(nbmax, 1) : 0);
        if (h->rows_ok) {
            int per_cu = 0;
            HIP_TRY(h, rows_occupancy(&per_cu, rows_lds_bytes(*h, 1, 1)));
            if (per_cu * h->num_cus < h->rG) h->rows_ok = false;
        }
        if (h->max_rows < 1 && !h->rows_ok)
            return fail(h, WRNN_EUNSUPPORTED, "these dims fit neither kernel's LDS layout with dense GRU weights "
                                              "(block-sparse 4x4 GRU weights would, see pruning.py)");
    }
    if (h->rows_ok) {
        std::vector<float> rslab((size_t)h->rG * h->rs.total);
        for (int w = 0; w < h->rG; ++w) pack_rows_slab(*h, w, rslab.data() + (size_t)w * h->rs.total);
        if (h->d_rslab) HIP_TRY(h, hipFree(h->d_rslab));
        HIP_TRY(h, hipMalloc(&h->d_rslab, rslab.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_rslab, rslab.data(), rslab.size() * 4, hipMemcpyHostToDevice));
        std::vector<float> Wt((size_t)h->rG * h->NT * rows_terms_kx(*h));
        if (rows_terms_composed(*h)) pack_terms_weights_composed(*h, Wt.data());
        else pack_terms_weights(*h, Wt.data());
        if (h->d_Wt) HIP_TRY(h, hipFree(h->d_Wt));
        HIP_TRY(h, hipMalloc(&h->d_Wt, Wt.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_Wt, Wt.data(), Wt.size() * 4, hipMemcpyHostToDevice));
    }
    if (h->g2.ok && !h->sparse) {
        PartScope ps(*h, h->g2, true);
        std::vector<float> rslab((size_t)h->rG * h->rs.total);
        for (int w = 0; w < h->rG; ++w) pack_rows_slab(*h, w, rslab.data() + (size_t)w * h->rs.total);
        if (h->d_rslab) HIP_TRY(h, hipFree(h->d_rslab));
        h->d_rslab = nullptr;
        HIP_TRY(h, hipMalloc(&h->d_rslab, rslab.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_rslab, rslab.data(), rslab.size() * 4, hipMemcpyHostToDevice));
        std::vector<float> Wt((size_t)h->rG * h->NT * rows_terms_kx(*h));
        if (rows_terms_composed(*h)) pack_terms_weights_composed(*h, Wt.data());
        else pack_terms_weights(*h, Wt.data());
        if (h->d_Wt) HIP_TRY(h, hipFree(h->d_Wt));
        h->d_Wt = nullptr;
        HIP_TRY(h, hipMalloc(&h->d_Wt, Wt.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_Wt, Wt.data(), Wt.size() * 4, hipMemcpyHostToDevice));
    }
    if (h->split_ok) {
        std::vector<float> gs, fs, Wt;
        pack_split_slabs(*h, gs, fs);
        pack_split_terms_weights(*h, Wt);
        for (auto pr : {std::make_pair(&h->d_sgslab, &gs), std::make_pair(&h->d_sfslab, &fs),
                        std::make_pair(&h->d_sWt, &Wt)}) {
            if (*pr.first) HIP_TRY(h, hipFree(*pr.first));
            *pr.first = nullptr;
            HIP_TRY(h, hipMalloc(pr.first, pr.second->size() * 4));
            HIP_TRY(h, hipMemcpy(*pr.first, pr.second->data(), pr.second->size() * 4, hipMemcpyHostToDevice));
        }
    }
    if (h->xcd_ok || h->xcdm_ok) {   // (the many-row kernel shares the terms GEMM; RAW has no xcd slab)
        std::vector<float> slab, Wt;
        if (h->xcd_ok) pack_xcd_slab(*h, slab);
        else slab.assign(4, 0.0f);
        pack_xcd_terms_weights(*h, Wt);
        for (auto pr : {std::make_pair(&h->d_xslab, &slab), std::make_pair(&h->d_xWt, &Wt)}) {
            if (*pr.first) HIP_TRY(h, hipFree(*pr.first));
            *pr.first = nullptr;
            HIP_TRY(h, hipMalloc(pr.first, pr.second->size() * 4));
            HIP_TRY(h, hipMemcpy(*pr.first, pr.second->data(), pr.second->size() * 4, hipMemcpyHostToDevice));
        }
    }
    if (h->xcdm_ok) {
        std::vector<float> slab, Wm;
        pack_xcdm_terms_weights(*h, Wm);
        if (h->d_xmWt) HIP_TRY(h, hipFree(h->d_xmWt));
        h->d_xmWt = nullptr;
        HIP_TRY(h, hipMalloc(&h->d_xmWt, Wm.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_xmWt, Wm.data(), Wm.size() * 4, hipMemcpyHostToDevice));
        pack_xcdm_slab(*h, slab);
        if (h->d_xmslab) HIP_TRY(h, hipFree(h->d_xmslab));
        h->d_xmslab = nullptr;
        HIP_TRY(h, hipMalloc(&h->d_xmslab, slab.size() * 4));
        HIP_TRY(h, hipMemcpy(h->d_xmslab, slab.data(), slab.size() * 4, hipMemcpyHostToDevice));
    }
    h->xcds_ok = false;
    if (h->xcds_cap) {
        const char *sp_env = std::getenv("WRNN_SPARSE");
        const int nbmax = (sp_env && std::string(sp_env) == "0") ? kSNB + 1 : xcds_nbmax(*h);
        if (h->sparse && nbmax <= kSNB) {
            std::vector<float> slab, Wt;
            pack_xcds_slab(*h, slab);
            pack_xcds_terms_weights(*h, Wt);
            for (auto pr : {std::make_pair(&h->d_xslab, &slab), std::make_pair(&h->d_xWt, &Wt)}) {
                if (*pr.first) HIP_TRY(h, hipFree(*pr.first));
                *pr.first = nullptr;
                HIP_TRY(h, hipMalloc(pr.first, pr.second->size() * 4));
                HIP_TRY(h, hipMemcpy(*pr.first, pr.second->data(), pr.second->size() * 4, hipMemcpyHostToDevice));
            }
            h->xcds_ok = true;
        }
    }
    h->ready = true;
    return WRNN_OK;
}

int wrnn_check(wrnn_t *h, void *stream) {
    if (!h) return WRNN_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    int ctl[kCtlWords];
    HIP_TRY(h, hipMemcpy(ctl, h->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    if (ctl[1] != 0) {
        static const char *lat_hops[] = {"q1", "h2", "f1", "f2", "logits", "gru1-terms", "gru1-terms"};
        static const char *row_hops[] = {"h1", "h2", "f1", "f2", "logits", "x"};
        const int hop = ctl[3];
        static const char *dm_hops[] = {"h_coarse", "o1", "coarse logits", "h_fine", "o3", "fine logits",
                                        "coarse label", "fine label"};
        static const char *split_hops[] = {"y", "f1", "f2", "h2", "h2", "gru1-terms", "gru1-terms"};
        static const char *xcd_hops[] = {"y", "f1", "f2", "h2", "gru1-terms", "gru1-terms"};
        static const char *xcdm_hops[] = {"h1", "y", "h2", "f1", "f2 (partial logits)", "x", "logits"};
        const int lp = h->last_path;
        const char *name = lp == 8 || lp == 3 || lp == 10 ? (hop >= 0 && hop < 8 ? dm_hops[hop] : "?")
                           : lp == 2 || lp == 9         ? (hop >= 0 && hop < 6 ? row_hops[hop] : "?")
                           : lp == 7                    ? (hop >= 0 && hop < 7 ? xcdm_hops[hop] : "?")
                           : lp >= 5                    ? (hop >= 0 && hop < 6 ? xcd_hops[hop] : "?")
                           : lp == 4                    ? (hop >= 0 && hop < 7 ? split_hops[hop] : "?")
                                                        : (hop >= 0 && hop < 7 ? lat_hops[hop] : "?");
        return fail(h, WRNN_ETIMEOUT,
                    "persistent kernel aborted: wait on hand-off '" + std::string(name) +
                        "' at step " + std::to_string(ctl[2]) + " in workgroup " + std::to_string(ctl[4]) +
                        " exceeded the timeout (grid not co-resident, or a fault)");
    }
    return WRNN_OK;
}

int wrnn_elapsed_ms(wrnn_t *h, float *ms) {
    if (!h || !ms) return WRNN_EINVAL;
    if (!h->timed) return fail(h, WRNN_EINVAL, "no wrnn_generate recorded yet");
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return WRNN_OK;
}

int wrnn_query(const wrnn_t *h, wrnn_info *info) {
    if (!h || !info) return WRNN_EINVAL;
    if (h->dm) {
        *info = wrnn_info{};
        info->grid = h->G;
        info->units_rnn = h->dmU;
        info->units_fc = h->dmUO;
        info->units_cls = h->dmUO2;
        info->lds_bytes = (int)dm_lds_bytes(*h, 1, 1);
        info->slab_floats = h->ds.total;
        info->num_cus = h->num_cus;
        info->rows_grid = h->G;
        info->rows_units_rnn = h->dmU;
        info->last_path = h->last_path;
        info->xcd_rows = h->dx_ok ? kDxRowsMax : 0;
        info->last_row_groups = h->last_row_groups;
        info->last_row_blocks = h->last_row_blocks;
        info->last_block_rows = h->last_block_rows;
        info->last_tile_rows = h->last_tile_rows;
        return WRNN_OK;
    }
    const bool rows_only = h->max_rows < 1;      // e.g. rnn 896 with block-sparse GRU weights
    info->grid = rows_only ? h->rG : h->G;
    info->units_rnn = rows_only ? h->rU : h->U;
    info->units_fc = rows_only ? h->rUF : h->UF;
    info->units_cls = rows_only ? h->rUC : h->UC;
    info->max_rows = h->max_rows;
    info->lds_bytes = (int)(rows_only ? rows_lds_bytes(*h, 1, 1) : lds_bytes_for(*h, h->max_rows));
    info->slab_floats = rows_only ? h->rs.total : h->s.total;
    info->rows_grid = h->rows_ok ? h->rG : 0;
    info->rows_units_rnn = h->rows_ok ? h->rU : 0;
    info->sparse_blocks = h->rows_ok ? h->rs.nbmax : 0;
    info->num_cus = h->num_cus;
    info->split_grid = h->split_ok ? h->sGg + h->sGf : 0;
    info->last_path = h->last_path;
    info->xcd_rows = (h->xcd_ok || h->xcds_ok) ? kXcds : 0;
    info->xcdm_rows = h->xcdm_ok ? kXcds * 4 * h->xcdm_nq : 0;
    info->last_row_groups = h->last_row_groups;
    info->last_row_blocks = h->last_row_blocks;
    info->last_block_rows = h->last_block_rows;
    info->last_tile_rows = h->last_tile_rows;
    return WRNN_OK;
}

const char *wrnn_last_error(const wrnn_t *h) { return h ? h->err.c_str() : "null handle"; }

int wrnn_philox_draws(uint64_t seed, int64_t row_offset, int rows, int step0, int steps, int K, int mode, float *out,
                      void *stream) {
    if (!out || rows < 1 || steps < 1 || K < 1 || step0 < 0)
        return cond_fail(WRNN_EINVAL, "need out, rows >= 1, steps >= 1, K >= 1, step0 >= 0");
    if (mode != WRNN_MODE_RAW && mode != WRNN_MODE_MOL && mode != WRNN_MODE_DM)
        return cond_fail(WRNN_EINVAL, "unknown mode");
    if ((long long)steps * rows * K > (1LL << 31) - 256) return cond_fail(WRNN_EINVAL, "too many draws for one call");
    if ((long long)step0 + steps > (1LL << 32)) return cond_fail(WRNN_EINVAL, "step index past 2^32");
    if (launch_philox_fill(out, seed, row_offset, rows, step0, steps, K, mode == WRNN_MODE_MOL ? 1 : 0,
                           (hipStream_t)stream) != hipSuccess)
        return cond_fail(WRNN_EHIP, "philox fill launch failed");
    return WRNN_OK;
}

void wrnn_destroy(wrnn_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (void *p : {(void *)h->d_slab, (void *)h->d_IW, (void *)h->d_Ib, (void *)h->d_cI, (void *)h->d_xg,
                    (void *)h->d_ctl, (void *)h->d_rslab, (void *)h->d_Wt, (void *)h->d_X, (void *)h->d_T,
                    (void *)h->d_act, (void *)h->d_state, (void *)h->d_flags, (void *)h->d_xr, (void *)h->d_dmslab,
                    (void *)h->d_dmflags, (void *)h->d_dmxg, (void *)h->d_sgslab, (void *)h->d_sfslab,
                    (void *)h->d_sWt, (void *)h->g2.d_slab, (void *)h->g2.d_Wt, (void *)h->dm2.d_slab,
                    (void *)h->d_gact, (void *)h->d_xslab, (void *)h->d_xWt, (void *)h->d_xstate, (void *)h->d_xgx,
                    (void *)h->d_members, (void *)h->d_xmslab, (void *)h->d_xmstate, (void *)h->d_xmxg, (void *)h->d_xmnoise,
                    (void *)h->d_xmWt, (void *)h->d_coef, (void *)h->d_FT, (void *)h->d_AT, (void *)h->d_frec,
                    (void *)h->d_cond,
                    (void *)h->d_dxslab, (void *)h->d_dxstate, (void *)h->d_dxnoise, (void *)h->d_dxxg,
                    (void *)h->d_larena, (void *)h->d_lstate, (void *)h->d_lxg})
        if (p) (void)hipFree(p);
    h->ltab.release();
    h->wtab.release();
    if (h->blas) (void)rocblas_destroy_handle(h->blas);
    delete h;
}
