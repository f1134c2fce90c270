// capi_cbhg.cpp — the C-ABI of the ragged Tacotron CBHGs (wrnn_cbhg_*; include/wavernn_amd.h).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "cbhg.h"
#include "condition.h"
#include "wavernn_amd.h"

using namespace wrnn;

namespace {

constexpr int kMaxRepack = 128;
constexpr int64_t kAlign = 64;   // floats: every section starts on a 256-byte boundary

int check_cfg(const wrnn_cbhg_cfg *c) {
    if (!c) return cond_fail(WRNN_EINVAL, "wrnn_cbhg: null cfg");
    const bool enc = c->K == 16 && c->in_channels == 128 && c->channels == 128 && c->proj1 == 128 && c->proj2 == 128 &&
                     c->pre_highway == 0 && c->highways == 4 && c->front == 1 && c->embed_dims == 256 && c->num_chars >= 1 &&
                     c->prenet_fc1 == 256 && c->tail_out == 256;
    const bool post = c->K == 8 && c->in_channels == 80 && c->channels == 128 && c->proj1 == 256 && c->proj2 == 80 &&
                      c->pre_highway == 1 && c->highways == 4 && c->front == 0 && c->tail_out >= 4 && c->tail_out % 4 == 0;
    if (enc || post) return WRNN_OK;
    return cond_fail(WRNN_EUNSUPPORTED,
                     "wrnn_cbhg: the kernels take the encoder CBHG (K 16, in 128, channels 128, projections 128/128, no "
                     "pre_highway, 4 highways, embedding 256 and prenet 256 -> 128 in front, tail 256) and the postnet CBHG "
                     "(K 8, in 80, channels 128, projections 256/80, pre_highway, 4 highways, no front, tail a multiple of 4); "
                     "got K " + std::to_string(c->K) + ", in " + std::to_string(c->in_channels) + ", channels " +
                         std::to_string(c->channels) + ", projections " + std::to_string(c->proj1) + "/" +
                         std::to_string(c->proj2) + ", pre_highway " + std::to_string(c->pre_highway) + ", highways " +
                         std::to_string(c->highways) + ", front " + std::to_string(c->front) + ", embedding " +
                         std::to_string(c->embed_dims) + ", prenet " + std::to_string(c->prenet_fc1) + ", tail " +
                         std::to_string(c->tail_out));
}

struct Plan {
    // sections of the scratch, in floats from its start
    int64_t table, bounds, offsets, order, packed, total;
    // packed weights, in floats from `packed`
    int64_t fc1, fc2, bank, bank_bn, p1, p1_bn, p2, p2_bn, prehw, hw[WRNN_CBHG_HIGHWAYS], hw_b[WRNN_CBHG_HIGHWAYS], gi, gi_b,
        bhh, tail;
    // stage buffers, in floats from the scratch's start
    int64_t front, fc1_out, bankbuf, pooled, p1_out, resid, hw_in, hw_t, hw_a, hw_b_buf, hw_out, gibuf, rnn;
    std::vector<cbhg::Repack> reps;
};

int64_t up(int64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

// `w` may be null: sizes and offsets only
Plan make_plan(const wrnn_cbhg_cfg &c, int64_t P, const wrnn_cbhg_weights *w) {
    Plan p{};
    const int C = c.channels, K = c.K;
    int64_t top = 0;
    auto take = [&](int64_t n) { const int64_t o = top; top += up(n); return o; };
    p.table = take((int64_t)kMaxRepack * sizeof(cbhg::Repack) / sizeof(float));
    p.bounds = take(2 * P);
    p.offsets = take(P + 1);
    p.order = take(P);
    p.packed = top;
    int64_t wtop = 0;
    auto wtake = [&](int64_t n) { const int64_t o = wtop; wtop += up(n); return o; };
    auto mat = [&](const float *src, int64_t dst, int O, int cin, int taps, int ld, int col0) {
        if (w) p.reps.push_back(cbhg::Repack{src, dst, O, cin, taps, ld, col0, 0});
    };
    auto vec = [&](const float *src, int64_t dst, int n) { mat(src, dst, n, 1, 1, n, 0); };
    auto bn = [&](int64_t dst, int O, const float *a, const float *b, const float *m, const float *v) {
        vec(a, dst, O), vec(b, dst + O, O), vec(m, dst + 2 * O, O), vec(v, dst + 3 * O, O);
    };
    if (c.front) {
        p.fc1 = wtake((int64_t)c.embed_dims * c.prenet_fc1);
        mat(w ? w->prenet_fc1_w : nullptr, p.fc1, c.prenet_fc1, c.embed_dims, 1, c.prenet_fc1, 0);
        p.fc2 = wtake((int64_t)c.prenet_fc1 * c.in_channels);
        mat(w ? w->prenet_fc2_w : nullptr, p.fc2, c.in_channels, c.prenet_fc1, 1, c.in_channels, 0);
    }
    p.bank = wtake((int64_t)c.in_channels * C * K * (K + 1) / 2);
    p.bank_bn = wtake((int64_t)K * 4 * C);
    for (int k = 0; k < K; ++k) {
        mat(w ? w->bank_w[k] : nullptr, p.bank + (int64_t)c.in_channels * C * k * (k + 1) / 2, C, c.in_channels, k + 1, C, 0);
        if (w) bn(p.bank_bn + (int64_t)k * 4 * C, C, w->bank_bn_w[k], w->bank_bn_b[k], w->bank_bn_mean[k], w->bank_bn_var[k]);
    }
    p.p1 = wtake((int64_t)3 * K * C * c.proj1);
    mat(w ? w->proj1_w : nullptr, p.p1, c.proj1, K * C, 3, c.proj1, 0);
    p.p1_bn = wtake(4 * c.proj1);
    if (w) bn(p.p1_bn, c.proj1, w->proj1_bn_w, w->proj1_bn_b, w->proj1_bn_mean, w->proj1_bn_var);
    p.p2 = wtake((int64_t)3 * c.proj1 * c.proj2);
    mat(w ? w->proj2_w : nullptr, p.p2, c.proj2, c.proj1, 3, c.proj2, 0);
    p.p2_bn = wtake(4 * c.proj2);
    if (w) bn(p.p2_bn, c.proj2, w->proj2_bn_w, w->proj2_bn_b, w->proj2_bn_mean, w->proj2_bn_var);
    if (c.pre_highway) {
        p.prehw = wtake((int64_t)c.proj2 * C);
        mat(w ? w->pre_highway_w : nullptr, p.prehw, C, c.proj2, 1, C, 0);
    }
    for (int i = 0; i < c.highways; ++i) {
        p.hw[i] = wtake((int64_t)C * 2 * C);
        p.hw_b[i] = wtake(2 * C);
        mat(w ? w->hw_w1[i] : nullptr, p.hw[i], C, C, 1, 2 * C, 0);
        mat(w ? w->hw_w2[i] : nullptr, p.hw[i], C, C, 1, 2 * C, C);
        vec(w ? w->hw_b1[i] : nullptr, p.hw_b[i], C);
        vec(w ? w->hw_b2[i] : nullptr, p.hw_b[i] + C, C);
    }
    p.gi = wtake((int64_t)C * 6 * C);
    p.gi_b = wtake(6 * C);
    p.bhh = wtake(6 * C);
    mat(w ? w->rnn_w_ih : nullptr, p.gi, 3 * C, C, 1, 6 * C, 0);
    mat(w ? w->rnn_w_ih_r : nullptr, p.gi, 3 * C, C, 1, 6 * C, 3 * C);
    vec(w ? w->rnn_b_ih : nullptr, p.gi_b, 3 * C);
    vec(w ? w->rnn_b_ih_r : nullptr, p.gi_b + 3 * C, 3 * C);
    vec(w ? w->rnn_b_hh : nullptr, p.bhh, 3 * C);
    vec(w ? w->rnn_b_hh_r : nullptr, p.bhh + 3 * C, 3 * C);
    p.tail = wtake((int64_t)2 * C * c.tail_out);
    mat(w ? w->tail_w : nullptr, p.tail, c.tail_out, 2 * C, 1, c.tail_out, 0);
    top += wtop;
    p.front = p.fc1_out = -1;
    if (c.front) {
        p.fc1_out = take(P * c.prenet_fc1);
        p.front = take(P * c.in_channels);
    }
    p.bankbuf = take(P * K * C);
    p.pooled = take(P * K * C);
    p.p1_out = take(P * c.proj1);
    p.resid = take(P * c.proj2);
    p.hw_in = c.pre_highway ? take(P * C) : p.resid;
    p.hw_t = take(P * 2 * C);
    p.hw_a = take(P * C);
    p.hw_b_buf = take(P * C);
    p.hw_out = c.highways % 2 ? p.hw_a : p.hw_b_buf;
    p.gibuf = take(P * 6 * C);
    p.rnn = take(P * 2 * C);
    p.total = top;
    return p;
}

bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" {

int wrnn_cbhg_supported(const wrnn_cbhg_cfg *cfg) { return check_cfg(cfg); }

int64_t wrnn_cbhg_scratch_bytes(const wrnn_cbhg_cfg *cfg, int64_t positions) {
    if (int rc = check_cfg(cfg)) return rc;
    if (positions < 1 || positions > (1 << 24)) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_scratch_bytes: positions outside 1..2^24");
    return make_plan(*cfg, positions, nullptr).total * (int64_t)sizeof(float);
}

int wrnn_cbhg_scratch_layout(const wrnn_cbhg_cfg *cfg, int64_t positions, int64_t *offsets) {
    if (int rc = check_cfg(cfg)) return rc;
    if (positions < 1 || positions > (1 << 24) || !offsets)
        return cond_fail(WRNN_EINVAL, "wrnn_cbhg_scratch_layout: positions outside 1..2^24 or null offsets");
    const Plan p = make_plan(*cfg, positions, nullptr);
    const int64_t o[WRNN_CBHG_STAGES] = {p.front, p.bankbuf, p.pooled, p.p1_out, p.resid, p.hw_in, p.hw_out, p.gibuf, p.rnn};
    for (int i = 0; i < WRNN_CBHG_STAGES; ++i) offsets[i] = o[i];
    return WRNN_OK;
}

int wrnn_cbhg_run(const wrnn_cbhg_cfg *cfg, const wrnn_cbhg_weights *w, const void *input, const int32_t *offsets,
                  int n_seq, float *out_rnn, float *out_proj, void *scratch, int64_t scratch_bytes, void *stream) {
    if (int rc = check_cfg(cfg)) return rc;
    const wrnn_cbhg_cfg &c = *cfg;
    if (!w || !input || !offsets || !out_proj || !scratch) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: null pointer");
    if (n_seq < 1) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: n_seq < 1");
    if (offsets[0] != 0) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: offsets[0] is not 0");
    for (int i = 0; i < n_seq; ++i)
        if (offsets[i + 1] <= offsets[i])
            return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: offsets[" + std::to_string(i + 1) +
                                              "] is not above its predecessor (every sentence has a position)");
    const int64_t P = offsets[n_seq];
    if (P > (1 << 24)) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: more than 2^24 positions");
    // required weight pointers: all but the parts this cfg has not
    {
        const float *const *wp = reinterpret_cast<const float *const *>(w);
        const float *const *lo_bank = &w->bank_w[0], *const *hi_bank = &w->bank_bn_var[WRNN_CBHG_MAX_K - 1] + 1;
        for (size_t i = 0; i < sizeof(*w) / sizeof(float *); ++i) {
            const float *const *f = wp + i;
            bool needed = true;
            if (f >= lo_bank && f < hi_bank) needed = (f - lo_bank) % WRNN_CBHG_MAX_K < c.K;
            if (f < lo_bank) needed = c.front != 0;
            if (f == &w->pre_highway_w) needed = c.pre_highway != 0;
            if (needed && (!*f || !aligned16(*f)))
                return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: weight pointer " + std::to_string(i) + " is null or not 16-byte aligned");
        }
    }
    if (!aligned16(input) || !aligned16(out_proj) || !aligned16(out_rnn) || (reinterpret_cast<uintptr_t>(scratch) & 255))
        return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: input / outputs need 16-byte, the scratch 256-byte alignment");
    Plan p = make_plan(c, P, w);
    if (scratch_bytes < p.total * (int64_t)sizeof(float))
        return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: scratch of " + std::to_string(scratch_bytes) + " bytes, " +
                                          std::to_string(p.total * sizeof(float)) + " needed");
    if ((int)p.reps.size() > kMaxRepack) return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: repack table overflow");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c.front) {   // an id beyond the embedding would read past it
        std::vector<int32_t> ids(P);
        if (hipMemcpyAsync(ids.data(), input, sizeof(int32_t) * P, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return cond_fail(WRNN_EHIP, "wrnn_cbhg_run: reading the ids failed");
        for (int64_t i = 0; i < P; ++i)
            if (ids[i] < 0 || ids[i] >= c.num_chars)
                return cond_fail(WRNN_EINVAL, "wrnn_cbhg_run: id " + std::to_string(ids[i]) + " at position " + std::to_string(i) +
                                                  " is outside the embedding's " + std::to_string(c.num_chars) + " rows");
    }
    // host tables: repack table, per-position sentence bounds, offsets, scan order (longest first)
    std::vector<float> blob(p.packed, 0.f);
    std::memcpy(blob.data() + p.table, p.reps.data(), p.reps.size() * sizeof(cbhg::Repack));
    int32_t *hb = reinterpret_cast<int32_t *>(blob.data() + p.bounds);
    for (int i = 0; i < n_seq; ++i)
        for (int q = offsets[i]; q < offsets[i + 1]; ++q) hb[2 * q] = offsets[i], hb[2 * q + 1] = offsets[i + 1];
    std::memcpy(blob.data() + p.offsets, offsets, sizeof(int32_t) * (n_seq + 1));
    int32_t *ho = reinterpret_cast<int32_t *>(blob.data() + p.order);
    std::iota(ho, ho + n_seq, 0);
    std::stable_sort(ho, ho + n_seq,
                     [&](int a, int b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });
    float *S = static_cast<float *>(scratch);
    if (hipMemcpyAsync(S, blob.data(), sizeof(float) * blob.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return cond_fail(WRNN_EHIP, "wrnn_cbhg_run: uploading the position tables failed");
    const int32_t *bounds = reinterpret_cast<const int32_t *>(S + p.bounds);
    float *W = S + p.packed;
    const int C = c.channels, K = c.K, Pi = (int)P;
    hipError_t e = cbhg::launch_repack(reinterpret_cast<const cbhg::Repack *>(S + p.table), (int)p.reps.size(), W, st);
    auto gemm = [&](const float *x, const int32_t *gather, int ldx, int cin, int taps, int64_t wt, int O, float *out, int ldo,
                    int mode, const float *bias, const float *bn, const float *res, int ldres, int bank) {
        if (e != hipSuccess) return;
        cbhg::Gemm g{};
        g.x = x, g.gather = gather, g.ldx = ldx, g.cin = cin, g.taps = taps, g.wt = W + wt, g.O = O, g.out = out, g.ldo = ldo;
        g.col0 = 0, g.mode = mode, g.bias = bias, g.bn = bn, g.res = res, g.ldres = ldres, g.bounds = bounds, g.P = Pi, g.bank = bank;
        e = cbhg::launch_gemm(g, st);
    };
    const float *x0 = static_cast<const float *>(input);
    if (c.front) {
        gemm(w->embedding, static_cast<const int32_t *>(input), c.embed_dims, c.embed_dims, 1, p.fc1, c.prenet_fc1,
             S + p.fc1_out, c.prenet_fc1, cbhg::kRelu, w->prenet_fc1_b, nullptr, nullptr, 0, 0);
        gemm(S + p.fc1_out, nullptr, c.prenet_fc1, c.prenet_fc1, 1, p.fc2, c.in_channels, S + p.front, c.in_channels, cbhg::kRelu,
             w->prenet_fc2_b, nullptr, nullptr, 0, 0);
        x0 = S + p.front;
    }
    gemm(x0, nullptr, c.in_channels, c.in_channels, 0, p.bank, C, S + p.bankbuf, K * C, cbhg::kReluBn, nullptr, W + p.bank_bn,
         nullptr, 0, K);
    if (e == hipSuccess) e = cbhg::launch_pool(S + p.bankbuf, S + p.pooled, K * C, bounds, Pi, st);
    gemm(S + p.pooled, nullptr, K * C, K * C, 3, p.p1, c.proj1, S + p.p1_out, c.proj1, cbhg::kReluBn, nullptr, W + p.p1_bn, nullptr,
         0, 0);
    gemm(S + p.p1_out, nullptr, c.proj1, c.proj1, 3, p.p2, c.proj2, S + p.resid, c.proj2, cbhg::kBnResidual, nullptr, W + p.p2_bn, x0,
         c.in_channels, 0);
    if (c.pre_highway)
        gemm(S + p.resid, nullptr, c.proj2, c.proj2, 1, p.prehw, C, S + p.hw_in, C, cbhg::kLinear, nullptr, nullptr, nullptr, 0, 0);
    const float *hx = S + p.hw_in;
    for (int i = 0; i < c.highways; ++i) {
        float *hy = S + (i % 2 ? p.hw_b_buf : p.hw_a);
        gemm(hx, nullptr, C, C, 1, p.hw[i], 2 * C, S + p.hw_t, 2 * C, cbhg::kLinear, W + p.hw_b[i], nullptr, nullptr, 0, 0);
        if (e == hipSuccess) e = cbhg::launch_highway(S + p.hw_t, hx, hy, Pi, st);
        hx = hy;
    }
    gemm(hx, nullptr, C, C, 1, p.gi, 6 * C, S + p.gibuf, 6 * C, cbhg::kLinear, W + p.gi_b, nullptr, nullptr, 0, 0);
    if (e == hipSuccess)
        e = cbhg::launch_gru_scan(S + p.gibuf, w->rnn_w_hh, w->rnn_w_hh_r, W + p.bhh, S + p.rnn,
                                  reinterpret_cast<const int32_t *>(S + p.order), reinterpret_cast<const int32_t *>(S + p.offsets),
                                  n_seq, st);
    gemm(S + p.rnn, nullptr, 2 * C, 2 * C, 1, p.tail, c.tail_out, out_proj, c.tail_out, cbhg::kLinear, nullptr, nullptr, nullptr, 0,
         0);
    if (e == hipSuccess && out_rnn)
        e = hipMemcpyAsync(out_rnn, S + p.rnn, sizeof(float) * P * 2 * C, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return cond_fail(WRNN_EHIP, std::string("wrnn_cbhg_run: launch: ") + hipGetErrorString(e));
    return WRNN_OK;
}

}  // extern "C"
