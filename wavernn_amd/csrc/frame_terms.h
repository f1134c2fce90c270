// frame_terms.h — records of the table-driven frame-term passes that are not part of a loop kernel's
// own row table (fatchord_xcdm.h: XcdmRow).
#pragma once

namespace wrnn {

// Folded lists (capi.cpp: wrnn_generate_list_folds): one record per launch row, parallel to the
// launch's XcdmRow table.  The row is one fold of an utterance of NF frames; launch step j is the
// utterance position pos0 + j (pos0 = fold·(target + overlap) + the fold-local first step of the
// launch), which lies past the utterance (fold_with_overlap's zero tail) from hop·NF on.
struct FoldRow {
    int pos0;
    int NF;
};

}  // namespace wrnn
