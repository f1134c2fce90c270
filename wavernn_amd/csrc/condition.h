// condition.h — what condition.hip defines for the host files beside the C-ABI of wavernn_amd.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>

namespace wrnn {

// the error text of a failed stateless call on this thread (wrnn_cond_last_error); returns `code`
int cond_fail(int code, const std::string &m);
// streaming sessions: the float64 post of the samples a push emits
hipError_t launch_postprocess_stream(const float *y, int U, int y_ld, int y_t0, int p0, int m, int wave_len,
                                     int fade_len, int mu_law, double mu, double *wave, int cap, hipStream_t st);

}  // namespace wrnn
