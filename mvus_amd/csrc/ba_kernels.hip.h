// HIP kernels of the BA hot path for gfx950 (MI355X, CDNA4).  fp64 throughout.
//
// Data layout in HBM (all SoA, camera-segmented, detections of one camera in frame order):
//   frame[M] u_raw[M] v_raw[M]            raw detections (common.py:1190)
//   u_obs[M] v_obs[M]                     observed pixel after the one-time undistortion (fixed calibration)
//   f[m]                                  residuals in the reference row order (common.py:476-485)
//   J[(chunk*2*NS + a*NS + k)*256 + lane] Jacobian slot k of row a (0:x, 1:y) of the lane-th detection of a chunk (chunk-major:
//                                         one contiguous 2*NS*2 KB block per workgroup, every store / load of a wavefront
//                                         one contiguous 512-B segment; see j_chunk_offset)
//   span[M]                               first active control point (global index), -1 = row is zero
// Work decomposition: one 256-thread workgroup (4 wavefronts of 64) per chunk of <=256 consecutive
// detections of ONE camera, so the camera's decoded parameters (R, t, K, d, alpha, beta, rs and the
// rotation-derivative matrix W) are wave-uniform and come through the scalar cache into SGPRs;
// consecutive lanes hold consecutive frames, i.e. neighbouring timestamps, so their knot-span
// searches and control-point gathers hit the same L1/L2 lines.

// This header has no code of its own: it names the stage headers.  A header that needs one stage includes that stage.
#pragma once
#include "ba_dev_problem.h"        // kThreads, DevProblem, the chunk-major Jacobian layout, the XCD tile map, cam_col
#include "ba_wave.hip.h"           // wave and DPP reductions, lds_barrier, last_block_done
#include "ba_observe.hip.h"        // k_cam_states, k_undistort_fixed, k_observations, k_pattern, k_motion, Jacobian export / freeze, outlier compaction
#include "ba_jop.hip.h"            // J v and the deterministic two-pass J^T u
#include "ba_vec.hip.h"            // BLAS-1: k_axpby, k_mul, k_fill, k_loss_weights, the two-stage dot product
#include "ba_lsmr.hip.h"           // the device-resident LSMR loop: k_lsmr_*, k_jvjtu
#include "ba_lm_trial.hip.h"       // the LM step's tail: k_lm_gnorm, k_lm_trial, k_lm_trial_sum
#include "ba_fd.hip.h"             // the finite-difference Jacobian: k_fd_*
