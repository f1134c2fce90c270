// frame_terms.h — records of the table-driven frame-term passes that are not part of a loop kernel's
// own row table (fatchord_xcdm.h: XcdmRow), and the host launchers of frame_terms.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "fatchord_xcdm.h"

namespace wrnn {

// Folded lists (capi_lists.cpp: wrnn_generate_list_folds): one record per launch row, parallel to the
// launch's XcdmRow table.  The row is one fold of an utterance of NF frames; launch step j is the
// utterance position pos0 + j (pos0 = fold·(target + overlap) + the fold-local first step of the
// launch), which lies past the utterance (fold_with_overlap's zero tail) from hop·NF on.
struct FoldRow {
    int pos0;
    int NF;
};

// host launchers (frame_terms.hip)
hipError_t launch_frame_cond(const float *mel, const float *aux, int U, int feat, int A4, int NF, int frames, int jlo,
                             int kind, float *rec, hipStream_t st);
hipError_t launch_terms_interp(const float *FT, const float *AT, const float *coef, float *T, int N, int U, int NF,
                               int NFF, int hop, int nJ, int nf, int stride, int b0, int nb, int t0, int nt,
                               hipStream_t st);
// streaming sessions: the windowed terms pass and the mel window
hipError_t launch_terms_interp_win(const float *FT, int ft_base, const float *AT, int at_base, const float *coef,
                                   float *T, int N, int U, int hop, int nJ, int t0, int nt, hipStream_t st);
hipError_t launch_stream_mel_window(const float *tail_old, const float *chunk, int U, int feat, int n, int R_old,
                                    int keep, int w0, int wn, float *win, float *tail_new, hipStream_t st);
// lists: the piece table of the lane list, the row tables of the wide and folded lists
hipError_t launch_terms_interp_list(const XcdPiece *pieces, int p0, int p1, int blocks, const float *coef, int N, int hop,
                                    int nJ, hipStream_t st);
int interp_list_blocks(int nt);
hipError_t launch_terms_interp_wide(const XcdmRow *rows, const float *coef, float *T, int N, int hop, int nJ, int nb,
                                    int nt, hipStream_t st);
hipError_t launch_terms_interp_folds(const XcdmRow *rows, const FoldRow *folds, const float *coef, float *T, int N,
                                     int hop, int nJ, int nb, int nt, hipStream_t st);

}  // namespace wrnn
