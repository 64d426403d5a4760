// The views the Schur kernels take by value and the failure codes they hand to the host: plain C++, shared by the device headers
// (ba_assemble*.hip.h, ba_band_*.hip.h, ba_sep.hip.h, ba_schur_product.hip.h, ba_rcs*.hip.h, ba_backsub.hip.h) and the host side.
#pragma once
#include <cmath>

namespace mvus {

constexpr int kNWin = 64;   // control points covered by a workgroup's LDS accumulation window

// N, N3 and every control-point index inside the kernels are LOCAL to this handle's slice, which starts at global
// control point row0 (0 and the whole spline unless the handle is a time shard)
struct NEView {
  double *A, *gc, *Cb, *gs, *Et;
  double* Apart;         // [assembly workgroups][8 wavefronts][(B+1)(B+2)/2] lower triangle of [camera slots; f] [..]^T, partial (k_cam_block_reduce sums them)
  int C, B, CB, N, N3, W;
  int row0;
  int* err;              // set when a row reaches outside the slice
};

// ---- partitioned (separator-based) parallel solve of the banded spline system ---------------------------
// The chain of control points is cut into P interiors of kPartL control points separated by separators of
// W-1 control points (= the block half-bandwidth, so two interiors never couple directly):
//     I_0 S_0 I_1 S_1 ... I_{P-1}
// A) every interior is factorised and solved independently (one wavefront per interior; one thread per
//    right-hand side, plus the 2*(W-1)*3 coupling columns V_p = B_p^-1 H[I_p,S_{p-1}], W_p = B_p^-1 H[I_p,S_p]);
// B) the separator system (block tridiagonal, blocks of 3(W-1)) is formed from short dot products;
// C) it is solved sequentially by one workgroup (P-1 small steps, all right-hand sides in parallel);
// D) the interiors are corrected: X_I = Y - V X_{S_{p-1}} - W X_{S_p}.

// Rows are LOCAL scalar rows of this handle's slice of the spline system (the whole system unless the handle is a
// time shard); separators are numbered GLOBALLY along the whole chain, 0 .. m-1.
struct PartView {
  int P;                 // interiors of this slice
  int s3;                // separator size in scalars, 3*(W-1)
  const int* i0;         // [P]  first scalar row of interior p
  const int* i1;         // [P]  one past the last scalar row of interior p
  const int* sl;         // [P]  first scalar row of the separator left of interior p (global number q_off+p-1), -1: none
  const int* sr;         // [P]  first scalar row of the separator right of interior p (global number q_off+p), -1: none
  int q_off;             // global number of the separator right of interior 0
  int m;                 // separators of the whole chain
  // separator tasks of k_part_reduce, [nt] each: row of the separator, interior left / right of it held here (-1: held
  // by the neighbouring shard, which adds that part), global number, own = this slice adds H(S,S) and the rhs rows
  int nt;
  const int *tc0, *tpl, *tpr, *tgq, *town;
  double* VW;            // [P][kPartRowsMax][2*s3]
  // one rank, round 5 (no back-correction of the interiors' columns, see HipSchur::band_chain):
  double* Dl;            // [m][s3][CB] a copy of the separators' reduced right-hand sides R_S (pv.R is solved in place); nullptr: not kept
  const double* Et;      // with Dl: the separators' rows of Z are ZERO and their own right-hand sides are read from the assembled blocks:
  const double* gs;      //   the camera-major cross block [C][N3][B] and the spline gradient [N3]
  const unsigned char* seprow;   // [N3] 1 = the row belongs to a separator
  int CB, B, N3;
  int direct;            // 1: no right-hand-side copy -- the interior solves read the assembled blocks (part_solve_block), Z's separator rows stay zero
  double* T;             // [m][s3][s3] diagonal blocks of the separator system
  double* U;             // [m][s3][s3] U[q] = T(q, q+1)
  double *U2, *Ha, *Hc;  // [m][s3][s3] each: cyclic-reduction workspace (k_sep_bcr_*)
  double* R;             // [m][s3][ncols] reduced right-hand sides -> solution of the separator system
};

struct BcrLevels { int nlev; int first[4]; int h[4]; };      // first[l]: block index of level l's survivor 0

// time shards: the two failure flags travel with the step (px[n], px[n+1]) through its sum over the ranks, so that every
// rank takes the same decision (a rank whose own interiors factorise fine must still see its neighbour's failure)
// A hand-over time-out of the reduced solve (fail[0] = kFailHandoverCode, ba_rcs.hip.h) is not a numerical failure: it travels as a
// value no sum of the other codes (<= 8 each, <= 64 ranks) can reach, and EVERY rank then reports the time-out -- all of them repeat
// the solve on the separate-launch route together (HipSchur::retry_same), none raises the damping alone.
// (round 6: packed by the last kernel of the solve, k_back_substitute; the sum is read where it lands -- by the trial kernel, which takes
// no step when any rank failed, and by the host through the driver's scalars: no pack / unpack launches, no copy of its own)
constexpr int kFailHandoverCode = 4;
constexpr double kFailHandoverSum = 1048576.0;
constexpr double kFailSpanSum = 4096.0;                 // flag bit 2 (a span table that does not belong to the point) in the sum of the second flags
inline int fail_sum_code(double t0) { return t0 >= kFailHandoverSum ? kFailHandoverCode : (t0 != 0.0 ? 8 : 0); }
inline int fail_sum_flag(double t1) { return (t1 >= kFailSpanSum ? 2 : 0) | (std::fmod(t1, kFailSpanSum) != 0.0 ? 1 : 0); }

}  // namespace mvus
