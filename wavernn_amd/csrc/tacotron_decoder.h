// tacotron_decoder.h — what tacotron_decoder.hip shares with its C-ABI host file (capi_taco.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include "wavernn_amd.h"

namespace wrnn {
namespace taco {

constexpr int kD = 256;      // decoder_dims = attention dims = encoder output dims
constexpr int kH = 512;      // lstm_dims
constexpr int kM = 80;       // n_mels
constexpr int kP1 = 256;     // prenet fc1
constexpr int kP2 = 128;     // prenet fc2
constexpr int kF = 32;       // LSA filters
constexpr int kTaps = 31;    // LSA kernel
constexpr int kMaxR = 20;
constexpr int kMaxRows = 128;
constexpr int kThreads = 256;
// state row layout (floats; step and stopped are int32 bit patterns)
constexpr int oAH = 0, oH1 = 256, oC1 = 768, oH2 = 1280, oC2 = 1792, oCTX = 2304, oFRAME = 2560, oSTEP = 2640,
              oSTOP = 2641, oCUM = 2644;
// scratch: 64 control words, then per-row activations
constexpr int kCtlWords = 64, kCounter = 32;
constexpr int sP = 0, sHN = 128, sX = 384, sX1 = 896, sX2 = 1408, sH1N = 1920, sH2N = 2432, kScratchRow = 2944;

struct Args {
    wrnn_taco_weights w;
    const float *enc, *proj;
    const int *t_enc;
    int t_max, rows, r;
    float thr;
    int step_cap, n_steps;
    float *state;
    int state_ld;
    float *mel, *attn, *scratch;
    long long timeout;
};

// one launch of `grid` workgroups (one per CU, all co-resident) on `st`
hipError_t launch_decoder_loop(const Args &a, int grid, hipStream_t st);

}  // namespace taco
}  // namespace wrnn
