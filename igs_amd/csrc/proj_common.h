// proj_common.h -- what the fused projections' forward and backward share (proj.hip, proj_bwd.hip): the size of a packed matrix and what
// the LDS lets a compute unit hold.  proj.hip states the tile layout.
#pragma once
#include "ffn_common.h"                   // the row loads and stores, the staging, the argument checks

#define PROJ_MAT (FFN_WM_TILES * MLP_TILE)                                       // elements of one packed matrix

template <typename T> struct ProjCfg {
    enum {
        HALF = AttnCfg<T>::HALF,
        QUARTER = PROJ_MAT / 4,                                                    // one output tile's four tiles
        PIECES = QUARTER * (int)sizeof(T) / 16 / FFN_THREADS,                      // a thread's 16-byte pieces of a quarter: 4 / 2
        GROUPS_PER_CU = HALF ? 2 : 1,                                              // what the LDS lets a compute unit hold
        WAVES_PER_SIMD = GROUPS_PER_CU * FFN_WAVES / 4,
    };
};
