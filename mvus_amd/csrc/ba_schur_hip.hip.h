// HIP implementation of the `Schur` concept of ba_schur.h: on-device assembly of the normal equations
// (camera blocks, block-banded spline block, cross block, gradient) from the slot Jacobian, and the
// damped solve by elimination of the spline block.
//
// Layout (one packed buffer `NE`; observation shards sum all of it, time shards only its head):
//   A  [C][B][B]        camera diagonal blocks, B = 3+P (alpha, beta, rs, camera params)
//   gc [C][B]           camera part of g = J^T f
//   (time shards only: the halo exchange buffer, diag(H) and g in x order -- the part summed over the ranks)
//   Cb [N][W][3][3]     Cb[g][w] = H[3g.., 3(g+w)..]: upper block band of the spline block, W >= 4
//   gs [3N]             spline part of g, internal order 3*ctrl + xyz
//   Et [C][3N][B]       cross block, camera-major: the control points a half chunk touches are one contiguous run of
//                       doubles per camera, so its flush is coalesced; k_build_rhs transposes it into the row-major
//                       [3N][C*B] right-hand-side / GEMM operand
// N here is the number of control points of the slice this handle holds: all of them, or -- time shard -- the owned
// range plus a halo on each side.
//
// This file is the umbrella: the device code lives in one header per stage, each of which compiles on its own
// (`make headers`).  The views and failure codes are ba_ne_views.h, the wavefront primitives ba_wave.hip.h.
//
// Assembly (HipSchur::assemble*): window-major, every entry stored once (ba_assemble_win.hip.h: k_assemble_windows, k_cam_block_sum) |
// MVUS_ASM_ATOMIC, MVUS_NE_FROM_J: detection-major (ba_assemble.hip.h: k_assemble_spans, k_cam_block_reduce); then the motion rows
// (k_det_motion | k_det_motion_wide | k_assemble_motion), the position priors' pass (ba_prior.hip.h: k_prior_ne) and the landmarks' pass
// (ba_landmark.hip.h: k_landmark_ne) where a handle carries them, k_freeze_ne, and on time shards k_halo_copy (ba_assemble.hip.h).
//
// Solve chain (HipSchur::solve_async), the default first and the switch of ba_switches.h that selects each alternative:
//   1. band pack, factorisation         ba_band_part.hip.h     k_band_pack, k_part_cholesky: the interior solves read their right-hand sides from the
//                                                               assembled blocks | MVUS_DIRECT_RHS=0: the copy Z = E beside the factorisation in
//                                                               k_cholesky_and_rhs | MVUS_NO_OVERLAP: k_build_rhs (pack and copy), k_part_cholesky
//   2. interiors                        ba_band_part.hip.h     k_part_solve, k_part_reduce (MVUS_PART_LEN: their length)
//      a band wider than six blocks     ba_band_generic.hip.h  k_band_chol_generic, k_band_solve_generic instead of 2. - 4.
//   3. separator system                 ba_sep.hip.h           cyclic reduction: k_sep_bcr_levels (MVUS_BCR_FUSED=0: k_sep_bcr_level each),
//                                                               k_bcr_tail_and_reduce_rhs | k_sep_bcr_tail, k_sep_bcr_rhs
//                                                               | MVUS_SEP_SEQUENTIAL: k_sep_factor, k_sep_rhs
//                                                               | time shards: k_sep2_build / reduce / finish (MVUS_SEP_TWO_LEVEL=0: one level)
//   4. interiors corrected              ba_band_part.hip.h     only with MVUS_PART_BACK: k_part_back; by default the product carries the separators'
//                                                               correction rows and one vector is corrected in 7.
//   5. Schur product                    ba_schur_product.hip.h k_schur_gemm on the fp64 matrix cores (MVUS_GEMM_SLABS: its K-slabs);
//                                                               time shards: k_sum_slabs
//   6. reduced camera system            ba_rcs.hip.h           blocked L D L^T: k_rcs_finish, k_rcs_factor (MVUS_RCS_TRSM=launch: + k_rcs_trsm),
//                                                               k_rcs_syrk, k_rcs_backsub
//                                       ba_rcs_gj.hip.h        | MVUS_RCS=gj: block Gauss-Jordan, k_schur_finish (ba_schur_product.hip.h), k_gj_step
//   7. back-substitution                ba_backsub.hip.h       k_back_substitute, k_back_correct
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ba_partition.h"
#include "ba_gemm_plan.h"
#include "ba_schur.h"

#include "ba_ne_views.h"
#include "ba_wave.hip.h"
#include "ba_assemble_win.hip.h"
#include "ba_assemble.hip.h"
#include "ba_landmark.hip.h"
#include "ba_band_generic.hip.h"
#include "ba_band_part.hip.h"
#include "ba_sep.hip.h"
#include "ba_schur_product.hip.h"
#include "ba_rcs.hip.h"
#include "ba_rcs_gj.hip.h"
#include "ba_backsub.hip.h"
