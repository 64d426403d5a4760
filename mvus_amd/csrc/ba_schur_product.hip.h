// The Schur product Et^T C^-1 Et on the fp64 matrix cores, the sum of its K-slabs and the reduced camera system S it leaves.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_gemm_plan.h"
#include "ba_ne_views.h"
#include "ba_wave.hip.h"

namespace mvus {

// (zero / nzero: the step vector every rank then writes its rows of, before it is summed -- cleared here, not by a launch of its own)
__global__ void k_sum_slabs(long long count, int nslab, const double* __restrict__ Gp, double* __restrict__ G0, double* __restrict__ zero, long long nzero) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < nzero) zero[i] = 0.0;
  if (i >= count) return;
  double t = 0.0;
  for (int sl = 0; sl < nslab; ++sl) t += Gp[sl * count + i];
  G0[i] = t;
}

// Gp[slab][CB][ncols] = Et^T Z over one K-slab: the one dense contraction of the solve (2 * CB^2 * 3N flops), on the
// fp64 matrix cores (v_mfma_f64_16x16x4_f64).  Both operands are K-major (the cross block camera-major, [C][3N][B]: row stride B and a per-lane column offset; Z [3N][ncols]), which is
// exactly the MFMA operand layout (lane l: A[l&15][k = l>>4], B[k = l>>4][l&15]; every 16-lane group reads 128
// contiguous bytes), so fragments go from global memory straight to registers -- no LDS staging.  One wavefront owns a
// 48x48 output tile (3x3 MFMA tiles, 36 accumulator registers) over wave_k rows of K; the four wavefronts of a
// workgroup take consecutive K ranges of the same tile and are summed through LDS.  Et^T C^-1 Et is symmetric: only
// 16x16 sub-blocks on or below the diagonal are computed (k_schur_finish and k_rcs_finish mirror).  In a tile ON the block
// diagonal that leaves three of the nine accumulators free -- (0,1), (0,2), (1,2) --, and they take the right-hand-side
// column: a fourth B fragment, column CB of the second operand, against the tile's three A fragments (ba_gemm_plan.h:
// gemm_sub).  So the column costs no tile, no matrix-core instruction and no read of an A strip of its own: nbk (nbk + 1) / 2
// tiles, nine useful sub-blocks each (it does cost the diagonal tiles a seventh fragment load per k-step: DESIGN 4.5).  Partial sums per slab are written, not atomically added: no memset, deterministic;
// the three sub-blocks above the diagonal of a diagonal tile are never written and never read.

// Operand sets of the Schur product: kGemmUn k-steps of a 48-wide A strip and NB B fragments of 16 columns (NB = 3: a 48-wide B
// strip; NB = 4, the diagonal tiles: + the rhs column), one double per lane and
// 16 x 4 fragment.  Two sets are alive: the loads of set k+1 are issued before the matrix-core instructions of set k
// (a lone wavefront per SIMD otherwise waits out the full memory latency once per set: 58 us instead of 27 at configs[2]).
template <int NB>
struct GemmSet {
  double a[kGemmUn][3], b[kGemmUn][NB];
  // ap / bp point at this lane's row (k + lane / 16) and first column; every address is inside the arrays (columns beyond the
  // matrix are clamped by the caller: they only feed output rows / columns that are never stored), so the loads carry no
  // predicate and no branch -- the steady-state loop below is one basic block and s_waitcnt can count the younger set's loads.
  __device__ __forceinline__ void load(const double* __restrict__ ap, const double* __restrict__ bp, long long lda, long long ldb,
                                       const int (&ao)[3], const int (&bo)[NB]) {
#pragma unroll
    for (int u = 0; u < kGemmUn; ++u) {
#pragma unroll
      for (int i = 0; i < 3; ++i) a[u][i] = ap[(long long)(4 * u) * lda + ao[i]];
#pragma unroll
      for (int j = 0; j < NB; ++j) b[u][j] = bp[(long long)(4 * u) * ldb + bo[j]];
    }
  }
  // the last, possibly partial set of the whole product: rows clamped to the last one, their values replaced by zero
  __device__ __forceinline__ void load_tail(const double* __restrict__ A, const double* __restrict__ B, long long lda, long long ldb,
                                            const int (&ao)[3], const int (&bo)[NB], int k, int k1, int lk) {
#pragma unroll
    for (int u = 0; u < kGemmUn; ++u) {
      const int row = k + 4 * u + lk;
      const bool kv = row < k1;
      const long long rc = kv ? row : k1 - 1;
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double v = A[rc * lda + ao[i]]; a[u][i] = kv ? v : 0.0; }
#pragma unroll
      for (int j = 0; j < NB; ++j) { const double v = B[rc * ldb + bo[j]]; b[u][j] = kv ? v : 0.0; }
    }
  }
  // NB = 3: all nine sub-blocks.  NB = 4: the six with j <= i, and a0, a1, a2 against the rhs fragment into (0,1), (0,2), (1,2)
  __device__ __forceinline__ void multiply(d4 (&acc)[3][3]) const {
#pragma unroll
    for (int u = 0; u < kGemmUn; ++u)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const GemmSub sb = gemm_sub(NB == 4, i, j);          // (folds: i, j are unrolled)
          if (sb.rhs) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][sb.rb], b[u][NB - 1], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
        }
  }
};

// sets [s_lo, s_hi) of 16 rows of ONE operand pair (A row stride lda with per-lane offsets ao, B row stride ldb with bo), rows
// [row_lo, row_hi): only the pair's very last set can be partial
template <int NB>
__device__ __forceinline__ void schur_gemm_sets(d4 (&acc)[3][3], const double* __restrict__ A, const double* __restrict__ Bm, long long lda, long long ldb,
                                                const int (&ao)[3], const int (&bo)[NB], int row_lo, int row_hi, int s_lo, int s_hi, int lk) {
  if (s_hi <= s_lo) return;
  const int nsets = (row_hi - row_lo + kGemmSetRows - 1) / kGemmSetRows;
  const bool tail = s_hi == nsets && (row_hi - row_lo) % kGemmSetRows != 0;
  const int nfull = s_hi - s_lo - (tail ? 1 : 0);
  const int k0 = row_lo + s_lo * kGemmSetRows;
  const double* ap = A + (long long)(k0 + lk) * lda;
  const double* bp = Bm + (long long)(k0 + lk) * ldb;
  const long long sa = kGemmSetRows * lda, sb = kGemmSetRows * ldb;
  GemmSet<NB> s0, s1;
  if (nfull > 0) {
    s0.load(ap, bp, lda, ldb, ao, bo);
    int si = 0;
    for (; si + 2 < nfull; si += 2) {                    // steady state: one basic block, every load unconditional
      s1.load(ap + sa, bp + sb, lda, ldb, ao, bo);
      s0.multiply(acc);
      ap += 2 * sa; bp += 2 * sb;
      s0.load(ap, bp, lda, ldb, ao, bo);
      s1.multiply(acc);
    }
    if (si + 1 < nfull) {
      s1.load(ap + sa, bp + sb, lda, ldb, ao, bo);
      s0.multiply(acc);
      s1.multiply(acc);
    } else {
      s0.multiply(acc);
    }
  }
  if (tail) {
    s0.load_tail(A, Bm, lda, ldb, ao, bo, row_lo + (s_hi - 1) * kGemmSetRows, row_hi, lk);
    s0.multiply(acc);
  }
}
// The product's K range is the rows [row_lo, row_hi) of (Ecm, Z) followed by the rows [0, sep_rows) of the compact pair (Dl, Xs) -- the
// separators' correction term (one rank, round 5; sep_rows = 0: none) --, cut into sets of 16; wavefront g of nslab * 4 takes sets
// [g q + min(g, r), ...) with q, r = nsets / nwaves, nsets % nwaves of the WHOLE range: every wavefront within one set of the others.
template <int NB>   // NB = 3: 48x48 tile below the block diagonal; NB = 4: tile on it, lower triangle + the rhs column (a0 == b0)
__device__ __forceinline__ void schur_gemm_tile(const NEView& ne, int ncols, const double* __restrict__ Ecm, const double* __restrict__ Z,
                                                double* __restrict__ Gp, int a0, int b0, int row_lo, int row_hi, int slab, int nslab, double* red,
                                                const double* __restrict__ Dl, const double* __restrict__ Xs, int sep_rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  d4 acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  int ao[3], ac[3], bo[NB];
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                // A = the cross block where the assembly left it (camera-major [C][3N][B]):
    const int col = min(a0 + 16 * i + lr, ne.CB - 1);          // column (c, k) of row r is Et[(c N3 + r) B + k] -- row stride B, per-lane offset
    ao[i] = (col / ne.B) * ne.N3 * ne.B + col % ne.B;
    ac[i] = col;                                               // (the compact pair is row-major [rows][CB])
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) bo[j] = j < 3 ? min(b0 + 16 * j + lr, ne.CB - 1) : ne.CB;      // (the rhs fragment: column CB of Z and of Xs in every lane)
  const int nmain = (row_hi - row_lo + kGemmSetRows - 1) / kGemmSetRows, ncorr = (sep_rows + kGemmSetRows - 1) / kGemmSetRows;
  const int nsets = nmain + ncorr, nwaves = nslab * 4, g = slab * 4 + wave;
  const int q = nsets / nwaves, r = nsets % nwaves;
  const int s_lo = g * q + min(g, r), s_hi = s_lo + q + (g < r ? 1 : 0);
  schur_gemm_sets<NB>(acc, Ecm, Z, ne.B, ncols, ao, bo, row_lo, row_hi, min(s_lo, nmain), min(s_hi, nmain), lk);
  if (ncorr > 0) schur_gemm_sets<NB>(acc, Dl, Xs, ne.CB, ncols, ac, bo, 0, sep_rows, max(s_lo, nmain) - nmain, max(s_hi, nmain) - nmain, lk);
  // sum the four wavefronts through LDS, then store: element (reg) of lane l of a 16x16 sub-block is its row (l>>4) + 4 reg, column l&15
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* dst = red + ((i * 3 + j) * 4 + r) * 64 + lane;
            *dst = (w == 0 ? 0.0 : *dst) + acc[i][j][r];
          }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < 9 * 4 * 64; e += 256) {
    const int l = e & 63, r = (e >> 6) & 3, ij = e >> 8;
    const GemmSub sb = gemm_sub(NB == 4, ij / 3, ij % 3);
    const int row = a0 + 16 * sb.rb + (l >> 4) + 4 * r;
    if (row >= ne.CB) continue;
    if (sb.rhs) {                                            // sixteen equal columns: the first one is G[row][CB]
      if ((l & 15) == 0) Gp[(long long)row * ncols + ne.CB] = red[e];
    } else {
      const int col = b0 + 16 * sb.cb + (l & 15);
      if (col < ne.CB) Gp[(long long)row * ncols + col] = red[e];
    }
  }
}

// Two workgroups per CU (<= 256 registers).  Every tile of a slab reads rows of the same K range, 12 tiles share each 48-column
// strip: all workgroups of a slab go to ONE XCD (workgroup L runs on XCD L % 8: slab = L % 8 + 8 * (L / 8 / tiles)), so a strip
// comes from HBM once and from that XCD's L2 afterwards (with the slabs dealt over all XCDs every XCD fetched every strip:
// 154 - 308 MB for 55 MB of operands, and the kernel ran at the fabric's rate, not the matrix cores').  Grid: 8 * tiles *
// ceil(nslab / 8) workgroups (gemm_grid); the slab count is chosen by the host (gemm_plan_slabs) to fill whole rounds of the XCD's slots.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_schur_gemm(NEView ne, int ncols, int row_lo, int row_hi, int nslab, const double* __restrict__ Ecm, const double* __restrict__ Z, double* __restrict__ Gp,
                  const double* __restrict__ Dl = nullptr, const double* __restrict__ Xs = nullptr, int sep_rows = 0) {
  __shared__ double red[9 * 4 * 64];
  const int tiles = gemm_tiles(ne.CB);
  const int L = blockIdx.x, j = L >> 3;
  const int slab = (L & 7) + 8 * (j / tiles), t = j % tiles;
  if (slab >= nslab) return;
  double* G = Gp + (long long)slab * ne.CB * ncols;
  // (Dl, Xs, sep_rows: one rank, round 5 -- the separators' share of E^T C^-1 E that is not in E_S^T X_S, (R_S - E_S)^T X_S over the compact
  // separator arrays, as further rows of K; with it the product may read the interiors' UNCORRECTED solutions: HipSchur, where ncorr is set)
  int bi, bj;
  gemm_tile_decode(t, bi, bj);
  if (bi == bj) schur_gemm_tile<4>(ne, ncols, Ecm, Z, G, bi * kGemmT, bj * kGemmT, row_lo, row_hi, slab, nslab, red, Dl, Xs, sep_rows);
  else schur_gemm_tile<3>(ne, ncols, Ecm, Z, G, bi * kGemmT, bj * kGemmT, row_lo, row_hi, slab, nslab, red, Dl, Xs, sep_rows);
}

// S = (A + lambda D_c) - sum_slabs Gp[:, :CB] (dense CB x CB, both triangles from the computed lower block triangle),
// rhs = gc - sum_slabs Gp[:, CB], in 32x32 tiles; the workgroup of tile (0,0) goes on to factorise the first pivot block of
// the Gauss-Jordan solve (ba_rcs_gj.hip.h), saving a launch.
constexpr int kNB = 32;
__device__ __forceinline__ void pivot_inverse_wave(double (*Dm)[kNB + 1], double* __restrict__ W, double* __restrict__ Pout, int* __restrict__ fail);
constexpr int kPivScratch = 5 * 16 * 17;      // doubles of LDS scratch pivot_inverse_wave needs
constexpr int kFinThreads = 256;            // 32x32 tile, four rows per thread (256 threads: the pivot inverse needs > 128 registers)
__global__ __launch_bounds__(kFinThreads) void k_schur_finish(NEView ne, int ncols, int nslab, double lambda, const double* __restrict__ Gp, double* __restrict__ S,
                                                             double* __restrict__ Linv, int* __restrict__ fail) {
  __shared__ double Dm[kNB][kNB + 1];
  __shared__ double Wp[kPivScratch];
  constexpr int kRowsPer = kNB * kNB / kFinThreads, kRowStep = kFinThreads / kNB;
  const int r0 = threadIdx.x / kNB, c = threadIdx.x % kNB;
  const int b = blockIdx.x * kNB + c;
  const long long stride = (long long)ne.CB * ncols;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;
  const int nb = min(kNB, ne.CB);
  // the slabs' partial sums: every load of a thread is independent of the others -- eight slabs x four rows in flight, added in
  // slab order (a loop of load, add, load ... is a chain of nslab memory round trips: 19 us of this kernel at 16 slabs)
  double gsum[kRowsPer];
  long long goff[kRowsPer];
#pragma unroll
  for (int q = 0; q < kRowsPer; ++q) {
    const int a = blockIdx.y * kNB + r0 + kRowStep * q;
    const int hi = a / 16 >= b / 16 ? a : b, lo = a / 16 >= b / 16 ? b : a;      // (k_schur_gemm computes the 16x16 sub-blocks on or below the diagonal)
    goff[q] = (a < ne.CB && b < ne.CB) ? (long long)hi * ncols + lo : -1;
    gsum[q] = 0.0;
  }
  for (int sl = 0; sl < nslab; sl += 8) {
    double t[8][kRowsPer];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < kRowsPer; ++q) t[u][q] = (sl + u < nslab && goff[q] >= 0) ? Gp[(sl + u) * stride + goff[q]] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < kRowsPer; ++q) gsum[q] += t[u][q];
  }
#pragma unroll
  for (int q = 0; q < kRowsPer; ++q) {
    const int r = r0 + kRowStep * q, a = blockIdx.y * kNB + r;
    double v = 0.0;
    if (a < ne.CB && b < ne.CB) {
      v = -gsum[q];
      if (a / ne.B == b / ne.B) {
        const int cam = a / ne.B;
        double h = ne.A[((long long)cam * ne.B + a % ne.B) * ne.B + b % ne.B];
        if (a == b) h += lambda * (h > 0.0 ? h : 1.0);
        v += h;
      }
      S[(long long)a * ne.CB + b] = v;
    }
    if (first) Dm[r][c] = (r < nb && c < nb && c <= r) ? v : ((r < nb && c < nb) ? 0.0 : (r == c ? 1.0 : 0.0));
  }
  if (blockIdx.y == 0 && r0 == 0 && b < ne.CB) {               // rhs rides as row CB
    double gr = 0.0;
    for (int sl = 0; sl < nslab; sl += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = sl + u < nslab ? Gp[(sl + u) * stride + (long long)b * ncols + ne.CB] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) gr += t[u];
    }
    S[(long long)ne.CB * ne.CB + b] = ne.gc[b] - gr;
  }
  if (!first) return;
  __syncthreads();
  if (threadIdx.x < 64) pivot_inverse_wave(Dm, Wp, Linv, fail);
}

}  // namespace mvus

// k_schur_finish runs the first pivot of the block Gauss-Jordan: the definition of pivot_inverse_wave (which needs kNB from here)
#include "ba_rcs_gj.hip.h"
