// capi_taco.cpp — the C-ABI of the Tacotron decoder loop (wrnn_taco_*; include/wavernn_amd.h).
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "condition.h"
#include "tacotron_decoder.h"
#include "wavernn_amd.h"

using namespace wrnn;

static int taco_check_cfg(const wrnn_taco_cfg *c) {
    if (!c) return cond_fail(WRNN_EINVAL, "wrnn_taco: null cfg");
    if (c->n_mels != taco::kM || c->decoder_dims != taco::kD || c->lstm_dims != taco::kH || c->encoder_dims != taco::kD ||
        c->prenet_fc1 != taco::kP1 || c->prenet_fc2 != taco::kP2 || c->lsa_filters != taco::kF ||
        c->lsa_kernel != taco::kTaps || c->max_r != taco::kMaxR)
        return cond_fail(WRNN_EUNSUPPORTED,
                         "wrnn_taco: the decoder kernel takes n_mels 80, decoder/encoder dims 256, lstm 512, prenet 256/128, "
                         "LSA 32 filters x 31 taps, max_r 20; got n_mels " + std::to_string(c->n_mels) + ", decoder " +
                             std::to_string(c->decoder_dims) + ", encoder " + std::to_string(c->encoder_dims) + ", lstm " +
                             std::to_string(c->lstm_dims));
    return WRNN_OK;
}

extern "C" {

int wrnn_taco_supported(const wrnn_taco_cfg *cfg) { return taco_check_cfg(cfg); }

int wrnn_taco_state_floats(const wrnn_taco_cfg *cfg, int t_max) {
    if (int rc = taco_check_cfg(cfg)) return rc;
    if (t_max < 1) return cond_fail(WRNN_EINVAL, "wrnn_taco_state_floats: t_max < 1");
    return taco::oCUM + 2 * t_max;
}

int wrnn_taco_state_layout(const wrnn_taco_cfg *cfg, int t_max, int32_t *offsets) {
    if (int rc = taco_check_cfg(cfg)) return rc;
    if (t_max < 1 || !offsets) return cond_fail(WRNN_EINVAL, "wrnn_taco_state_layout: t_max < 1 or null offsets");
    const int o[WRNN_TACO_STATE_FIELDS] = {taco::oAH,   taco::oH1,   taco::oC1,  taco::oH2, taco::oC2,           taco::oCTX,
                                           taco::oCUM, taco::oCUM + t_max, taco::oFRAME, taco::oSTEP, taco::oSTOP};
    for (int i = 0; i < WRNN_TACO_STATE_FIELDS; ++i) offsets[i] = o[i];
    return WRNN_OK;
}

int64_t wrnn_taco_scratch_floats(const wrnn_taco_cfg *cfg, int rows) {
    if (int rc = taco_check_cfg(cfg)) return rc;
    if (rows < 1 || rows > taco::kMaxRows) return cond_fail(WRNN_EINVAL, "wrnn_taco_scratch_floats: rows outside 1..128");
    return taco::kCtlWords + (int64_t)rows * taco::kScratchRow;
}

int wrnn_taco_run(const wrnn_taco_cfg *cfg, const wrnn_taco_weights *w, const float *enc, const float *enc_proj,
                  const int32_t *t_enc, int t_max, int rows, int r, float stop_threshold, int step_cap, int n_steps,
                  float *state, float *mel, float *attn, float *scratch, int timeout_ms, void *stream) {
    if (int rc = taco_check_cfg(cfg)) return rc;
    if (!w || !enc || !enc_proj || !t_enc || !state || !mel || !attn || !scratch)
        return cond_fail(WRNN_EINVAL, "wrnn_taco_run: null pointer");
    const float *const *wp = reinterpret_cast<const float *const *>(w);
    for (size_t i = 0; i < sizeof(*w) / sizeof(float *); ++i)
        if (!wp[i]) return cond_fail(WRNN_EINVAL, "wrnn_taco_run: weight pointer " + std::to_string(i) + " is null");
    if (rows < 1 || rows > taco::kMaxRows) return cond_fail(WRNN_EINVAL, "wrnn_taco_run: rows outside 1..128");
    if (r < 1 || r > taco::kMaxR) return cond_fail(WRNN_EINVAL, "wrnn_taco_run: r outside 1..20");
    if (t_max < 1 || step_cap < 1 || n_steps < 0) return cond_fail(WRNN_EINVAL, "wrnn_taco_run: t_max / step_cap < 1 or n_steps < 0");
    if (n_steps == 0) return WRNN_OK;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return cond_fail(WRNN_EHIP, "wrnn_taco_run: no device");
    if (cus < taco::kMaxRows)
        return cond_fail(WRNN_EUNSUPPORTED, "wrnn_taco_run: needs at least 128 CUs (one workgroup per CU, one owner per row)");
    const int G = cus < 256 ? taco::kMaxRows : 256;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the rows' lengths are checked on the host: a length beyond t_max would index past the buffers
    std::vector<int32_t> te(rows);
    if (hipMemcpyAsync(te.data(), t_enc, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return cond_fail(WRNN_EHIP, "wrnn_taco_run: reading t_enc failed");
    for (int b = 0; b < rows; ++b)
        if (te[b] < 1 || te[b] > t_max)
            return cond_fail(WRNN_EINVAL, "wrnn_taco_run: t_enc[" + std::to_string(b) + "] outside 1..t_max");
    if (hipMemsetAsync(scratch, 0, sizeof(unsigned) * taco::kCtlWords, st) != hipSuccess)
        return cond_fail(WRNN_EHIP, "wrnn_taco_run: hipMemsetAsync failed");
    taco::Args a;
    a.w = *w;
    a.enc = enc;
    a.proj = enc_proj;
    a.t_enc = t_enc;
    a.t_max = t_max;
    a.rows = rows;
    a.r = r;
    a.thr = stop_threshold;
    a.step_cap = step_cap;
    a.n_steps = n_steps;
    a.state = state;
    a.state_ld = taco::oCUM + 2 * t_max;
    a.mel = mel;
    a.attn = attn;
    a.scratch = scratch;
    a.timeout = (long long)(timeout_ms > 0 ? timeout_ms : 2000) * 100000ll;  // 100 MHz realtime counter
    if (hipError_t e = taco::launch_decoder_loop(a, G, st); e != hipSuccess)
        return cond_fail(WRNN_EHIP, std::string("wrnn_taco_run: launch: ") + hipGetErrorString(e));
    unsigned ctl[4] = {0, 0, 0, 0};
    if (hipError_t e = hipMemcpyAsync(ctl, scratch, sizeof(ctl), hipMemcpyDeviceToHost, st); e != hipSuccess)
        return cond_fail(WRNN_EHIP, std::string("wrnn_taco_run: ") + hipGetErrorString(e));
    if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess)
        return cond_fail(WRNN_EHIP, std::string("wrnn_taco_run: ") + hipGetErrorString(e));
    if (ctl[0] != 0)
        return cond_fail(WRNN_ETIMEOUT, "wrnn_taco_run: grid barrier timed out at step " + std::to_string(ctl[1]) + ", phase " +
                                            std::to_string(ctl[2]) + ", workgroup " + std::to_string(ctl[3]));
    return WRNN_OK;
}

}  // extern "C"
