// hb_sbayes_sparse.hpp — what hb_sbayes.hip (the host loop) and hb_sbayes_sparse.hip (the kernels) share of the summary-level
// sampler on a sparse LD matrix: SBayesS() of the reference (src/SBayesS.cpp:277-600) from the handle's device CSC.
#pragma once
#include "hb_internal.hpp"
#include "hb_ldm.hpp"

#define SS_GS HB_LDM_GS // markers per k_ss_group launch (= its workgroup size); the handle's per-marker runs are cut for it

// Philox purpose 4 (HB_PURPOSE_REDRAW, hb_rng.hpp): the normals of the truncation's redraws. Redraw k = 1 .. 101 of marker j in
// sweep `iter` is block j * SS_REDRAW_BLK + k of the stream sub = (4 << 56) | iter.
#define SS_REDRAW_BLK 128ull

// device buffers of one sparse run: hb_sb_dev's (b.ldm stays null) and what SBayesS() has beyond SBayesD()
struct hb_ss_dev {
    hb_sb_dev b;
    hb_ldm_csc csc;
    double *varediff = nullptr; // [m_pad] (m - nnz(column i)) / m, :131-141
    double *varei = nullptr;    // [m_pad] this sweep's varediff[i] * vara + vare (k_ss_pre)
    double *sgn = nullptr;      // [m_pad] this sweep's sign of 2 v varei per marker (k_ss_pre; -1 only after a negative variance draw)
    double *vxt = nullptr;      // [m_pad] ldm[i][i]: the truncation's vx (b.vx is the "has statistics" word)
    double *ex = nullptr;       // [2] this sweep's vara, and vary
    double *gtab = nullptr;     // [SS_GS] n (g_old - g_new) of the current group by position, 0 where nothing moved
    double *rd = nullptr;       // [2] the sweep's last redrawn marker (-1: none) and its last draw squared (:392)
    int32_t *cursor = nullptr;  // [m_pad] entries of column j below the current group's rows (k_ss_update's place in its row)
};
int hbk_ss_enqueue_sweep(hb_ss_dev *d, int model, int n_fold);
int hbk_ss_windows(hb_ss_dev *d);
int hbk_ss_varediff(hb_ss_dev *d);
