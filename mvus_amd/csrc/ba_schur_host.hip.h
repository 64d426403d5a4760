// Host side of the LM + Schur path: HipSchur owns the normal-equation storage, the partition tables, the cost models for the window
// length and the slab count, and every launch of the kernels behind ba_schur_hip.hip.h (included first: the umbrella of the stage headers, where the device code lives).
#pragma once
#include "api_common.h"      // HipError, MVUS_HIP, RoctxRange
#include "ba_dev_problem.h"
#include "ba_held.h"
#include "ba_problem.h"
#include "ba_schur_hip.hip.h"
#include "ba_switches.h"

namespace mvus {

// Everything a HipSchur takes from the backend's pool and from the device, given back by the destructor: the first member of HipSchur,
// so a constructor that throws half-way (any MVUS_HIP after the first allocation) leaks nothing
template <class BE>
struct SchurOwner {
  BE& be;
  std::vector<double*> pool;
  DeviceOwner mem;
  explicit SchurOwner(BE& b) : be(b) {}
  SchurOwner(const SchurOwner&) = delete;      // (alloc makes room in its list first, like DeviceOwner: nothing throws between taking and recording)
  double* alloc(size_t len) { pool.reserve(pool.size() + 1); pool.push_back(be.alloc((int64_t)len)); return pool.back(); }
  template <class T> T* device(size_t count) { return mem.device<T>(count); }
  template <class T> T* mapped(size_t count) { return mem.mapped<T>(count); }
  ~SchurOwner() { for (double* p : pool) be.release(p); }
};

// column batch and dynamic LDS of k_sep_bcr_rhs for a chain of m separators: kBcrCols columns per workgroup, one where they exceed 64 KB
// (a chain too long even for one column keeps the sequential separator kernels: HipSchur::use_bcr)
struct BcrPlan { int cols = kBcrCols; size_t lds = 0; };
inline BcrPlan bcr_plan(int m, int s3) {
  BcrPlan p;
  p.lds = (size_t)2 * std::max(m, 1) * s3 * p.cols * sizeof(double);
  if (p.lds > 64 * 1024) { p.cols = 1; p.lds /= kBcrCols; }
  return p;
}

// hands out byte offsets one behind the other (the tables of one allocation); `at` ends as the total size
struct Bump { size_t at = 0; size_t take(size_t bytes) { const size_t o = at; at += bytes; return o; } };

template <class BE>
struct HipSchur {
  SchurOwner<BE> own;       // first member: destroyed last, and also when the constructor throws
  BE& be;
  const Switches sw;        // ba_switches.h: read once, here
  NEView ne{};
  int ncols = 0, BW = 0;
  size_t ne_count = 0;
  double* NEset[2] = {nullptr, nullptr};   // two sets of normal-equation blocks: the solver reads NEset[ne_cur]; the other one takes the speculative linearisation (linearize_spec)
  int ne_cur = 0;
  size_t off_gc = 0, off_Cb = 0, off_gs = 0, off_Et = 0, off_Apart = 0;
  double *NE = nullptr, *Lb = nullptr, *Z = nullptr, *G = nullptr, *G0 = nullptr, *pc = nullptr,
         *D = nullptr, *gx = nullptr, *px = nullptr, *sepbuf = nullptr;
  double *S = nullptr, *S2 = nullptr, *Linv = nullptr;   // workspace of the block Gauss-Jordan: allocated under MVUS_RCS=gj only
  RcsView rcs{};            // reduced camera system in block-image form (ba_rcs.hip.h)
  unsigned* rcs_flags = nullptr;   // step counter of the in-launch hand-over (k_rcs_factor -> its row workgroups); zeroed by k_rcs_finish
  bool rcs_trsm_launch = sw.rcs_trsm_launch; // MVUS_RCS_TRSM=launch, or switched on for good by retry_same
  bool bcr_fused = sw.bcr_fused;             // the wide cyclic-reduction levels in one launch (k_sep_bcr_levels); MVUS_BCR_FUSED=0: a launch per level
  unsigned* bcr_done = nullptr;              // [m] per separator: the level mark of the hand-over
  unsigned bcr_epoch = 0;
  unsigned rcs_spin_limit = sw.rcs_spin_limit >= 0 ? (unsigned)sw.rcs_spin_limit : kRcsSpinLimit;   // MVUS_RCS_SPIN_LIMIT: test hook (0 = the first poll that finds the flag behind gives up)
  int part_len = kPartL;    // control points per interior of the band solver (<= kPartL)
  int* fail = nullptr;      // [0] numerical failure of a solve, [1] a row reached outside the slice (assembly)
  int* fail_host = nullptr;
  int* fail_map = nullptr;  // device address of fail_host (mapped pinned)
  PartView pv{};
  int nslab = 1;            // K-slabs of the Schur product (partial sums in G): HipSchur::plan_gemm
  int ncorr = 0;            // 1: the product carries the separators' correction term and the interiors are NOT back-corrected
  int n_own_sep = 0;        // separators of this slice (a time shard adds the correction rows of ITS separators: every separator once over the ranks)
  // time shards, round 6: two-level elimination of the separators (k_sep2_*): the local ones by this rank alone, the world - 1 cut separators summed
  bool two_level = false;
  int k_loc = 0, has_ghost = 0, has_cut = 0, ncut = 0;
  double *Rloc = nullptr, *CGK = nullptr, *cutbuf = nullptr, *cutws = nullptr;
  size_t cut_count = 0;
  BcrPlan bcr{}, bcr_loc{}, bcr_cut{};   // k_sep_bcr_rhs of the whole chain, of a time shard's local chain, of the cut system
  bool use_bcr = false;     // cyclic reduction; the sequential separator kernels remain for chains too long for its LDS (and MVUS_SEP_SEQUENTIAL)
  // slice of the spline system held by this handle (everything unless it is a time shard)
  bool shard = false;
  int Ntot = 0, own_lo = 0, own_hi = 0;        // owned control points, LOCAL indices (slice starts at ne.row0)
  size_t sep_count = 0, halo_count = 0, nAg = 0, n_apart = 0;
  int nbound = 0;
  bool diag_pending = false;                   // D / g in x order still to be written (folded into the next k_build_rhs)
  bool overlap_chol = true;                    // interiors factorised beside the right-hand-side copies (k_cholesky_and_rhs); MVUS_NO_OVERLAP, wide bands: not
  int rhs_tiles_z = 0;
  int* halo_tables = nullptr;                  // [nbound] cut, [nbound] index in the packed buffer
  // window-major fused assembly (ba_assemble_win.hip.h): tables and the per-(window, camera) camera-block partials
  WinView wv{};
  bool use_win = false;
  bool wide = false;                           // band wider than six control points: the general band kernels instead of the partitioned solver
  size_t win_lds = 0;

  // K-slabs of the Schur product: the cost model of ba_gemm_plan.h for this device's CU count (MVUS_GEMM_SLABS: a forced count)
  void plan_gemm(int rows) {
    int cus = 256;
    { int dev = 0; hipDeviceProp_t pr{}; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount; }
    nslab = gemm_plan_slabs(ne.CB, rows, cus, sw.gemm_slabs);
  }

  explicit HipSchur(BE& b) : own(b), be(b), sw(read_switches()) {
    plan_slice();                          // (every refusal is thrown here, before anything is allocated)
    alloc_workspace();
    plan_partition();
    plan_separators();
    plan_two_level();
    win_prepare();
  }
  int sctrl() const { return ne.W - 1; }   // control points of a separator
  // slice of the spline system, band width, layout of the packed normal equations
  void plan_slice() {
    const HostProblem& hp = be.hp;
    const auto& ts = be.tshard;
    shard = ts.on && ts.world > 1;
    Ntot = hp.N;
    int glo = 0, ghi = hp.N, olo = 0, ohi = hp.N;          // slice and owned range, global control points
    if (shard) {
      olo = ts.cuts[ts.rank]; ohi = ts.cuts[ts.rank + 1];
      glo = std::max(0, olo - ts.halo); ghi = std::min(hp.N, ohi + ts.halo);
    }
    ne.C = hp.C; ne.B = 3 + hp.P; ne.CB = ne.C * ne.B; ne.N = ghi - glo; ne.N3 = 3 * ne.N; ne.row0 = glo;
    own_lo = olo - glo; own_hi = ohi - glo;
    int W = 4;
    for (int j = 1; j + 1 < hp.T; ++j) {
      if (hp.ms_part[j] < 0 || hp.ms_part[j - 1] != hp.ms_part[j]) continue;
      int lo = std::min(hp.ms_ctrl[j - 1], hp.ms_ctrl[j]), hi = std::max(hp.ms_ctrl[j - 1], hp.ms_ctrl[j]);
      if (hp.motion_type == MVUS_MOTION_F && hp.ms_part[j + 1] == hp.ms_part[j]) { lo = std::min(lo, hp.ms_ctrl[j + 1]); hi = std::max(hi, hp.ms_ctrl[j + 1]); }
      W = std::max(W, hi + 3 - lo + 1);
    }
    // W <= 6: the partitioned band solver (templates for W = 4 and 6).  Wider -- FITPACK knots less than a frame apart, the motion
    // rows then reach over more than three knot spans -- : the band as it is, factorised and solved by the general kernels
    // (k_band_chol_generic / k_band_solve_generic: one CU, for the small problems of the incremental loop where this happens)
    if (W > kWideW) throw HipError{"LM_SCHUR: motion rows couple control points " + std::to_string(W) + " apart (knots far below one frame) - unsupported band width (at most " + std::to_string(kWideW) + ")", MVUS_E_UNSUPPORTED};
    wide = W > 6;
    if (wide && shard) throw HipError{"LM_SCHUR: a band wider than six control points is not supported on a time shard", MVUS_E_UNSUPPORTED};
    if (!wide) W = W <= 4 ? 4 : 6;
    ne.W = W;
    BW = 3 * W - 1;
    ncols = ne.CB + 1;
    overlap_chol = !sw.no_overlap && !wide;
    if (shard) {
      if (ts.halo < sctrl() + 3) throw HipError{"time shard: halo must be at least band half-width + 3 control points"};
      for (int r = 0; r < ts.world; ++r)
        if (ts.cuts[r + 1] - ts.cuts[r] < 2 * ts.halo + sctrl() + 1) throw HipError{"time shard: a rank owns fewer control points than 2 * halo + separator"};
    }
    // packed normal equations [A | gc | (halo exchange buffer) | Cb | gs | Et]: the head is what a time shard sums over the ranks
    nbound = shard ? (ts.rank > 0) + (ts.rank + 1 < ts.world) : 0;
    halo_count = shard ? (size_t)(ts.world - 1) * 2 * ts.halo * (3 * ne.CB + W * 9 + 3) : 0;
    const size_t nA = (size_t)ne.C * ne.B * ne.B, ngc = ne.CB, nCb = (size_t)ne.N * W * 9, ngs = ne.N3, nEt = (size_t)ne.N3 * ne.CB;
    nAg = nA + ngc;
    // time shards: diag(H) and g ride in the summed head too ([A | gc | halo | D | g])
    const size_t ndg = shard ? 2 * (size_t)hp.n : 0;
    ne_count = nA + ngc + halo_count + ndg + nCb + ngs + nEt;
    // + the per-workgroup camera-block partials of the assembly, behind the blocks (cleared with them, never summed over ranks)
    n_apart = (size_t)kGaParts * (kGaThreads / 64) * std::max<size_t>(hp.chunks.size(), 1) * (size_t)((ne.B + 1) * (ne.B + 2) / 2);
    off_gc = nA; off_Cb = nA + ngc + halo_count + ndg; off_gs = off_Cb + nCb; off_Et = off_gs + ngs; off_Apart = off_Et + nEt;
  }
  // the blocks, the band solver's and the reduced camera system's workspace, the failure flags
  void alloc_workspace() {
    const HostProblem& hp = be.hp;
    NEset[0] = own.alloc(ne_count + n_apart);
    bind_ne(0);
    Lb = own.alloc((size_t)ne.N3 * (BW + 1));
    Z = own.alloc((size_t)ne.N3 * ncols);
    plan_gemm(3 * (own_hi - own_lo));
    G = own.alloc((size_t)nslab * ne.CB * ncols);
    G0 = own.alloc((size_t)ne.CB * ncols);
    pc = own.alloc(ne.CB);
    // which solver of the reduced camera system: the blocked L D L^T of ba_rcs.hip.h (round 5) at every size -- one launch up to 144
    // unknowns (24 us against the block Gauss-Jordan's 32 at 63 unknowns), and with the rows below each super-block solved inside the
    // factor launch it is level with or ahead of the Gauss-Jordan beyond (configs[2]: 0.488 - 0.495 against 0.498 - 0.503 ms per
    // step, configs[3]: 1.297 against 1.299).  MVUS_RCS=gj keeps the Gauss-Jordan (A/B, tests) and its workspace.
    if (sw.rcs_gj) {
      S = own.alloc((size_t)(ne.CB + 1) * ne.CB);
      S2 = own.alloc((size_t)(ne.CB + 1) * ne.CB);
      Linv = own.alloc((size_t)((ne.CB + kNB - 1) / kNB) * kNB * kNB);
    }
    rcs.nn = ne.CB; rcs.nbk = (ne.CB + 15) / 16;
    rcs.Simg = own.alloc(rcs_doubles(ne.CB)); rcs.Tsc = own.alloc(rcs_doubles(ne.CB)); rcs.x = own.alloc((size_t)rcs.nbk * 16);
    rcs_flags = own.template device<unsigned>(4);
    MVUS_HIP(hipMemsetAsync(rcs_flags, 0, 4 * sizeof(unsigned), be.stream));
    MVUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rcs_trsm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)((rcs_stage_doubles(kRcsSP) + 512) * sizeof(double))));
    MVUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rcs_backsub), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(rcs_backsub_doubles(rcs.nbk) * sizeof(double))));
    if (!shard) { D = own.alloc(2 * (size_t)hp.n); gx = D + hp.n; }      // (a time shard's ride in the summed head: bind_ne)
    px = own.alloc(hp.n + 2);                         // + the two failure flags of a time shard
    fail = own.template device<int>(4);              // [2]: sticky hand-over time-out mark of the running solve
    MVUS_HIP(hipMemsetAsync(fail, 0, 4 * sizeof(int), be.stream));
    fail_host = own.template mapped<int>(2);
    fail_host[0] = fail_host[1] = 0;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&fail_map), fail_host, 0) != hipSuccess) fail_map = nullptr;
    ne.err = fail + 1;
  }
  // partition of the owned chain into interiors and separators, its tables on the device; a time shard's halo tables
  void plan_partition() {
    const auto& ts = be.tshard;
    // the separators are numbered along the chain of ALL ranks (each rank can compute every other rank's count from the cuts)
    const bool close = shard && ts.rank + 1 < ts.world;
    // Interior length: the factorisation of an interior is one dependent chain of its rows (0.3 us a row), the separator system one of
    // log2(separators) levels whose cost grows with the number of right-hand-side columns.  Few columns (<= 128: configs[1], [4]):
    // half-length interiors -- measured 0.333 -> 0.309 ms and 0.390 -> 0.362 ms a step; 289 columns: no difference; 577: 1.283 -> 1.363.
    // (Every rank of a sharded solve computes the same value: CB is global.)
    part_len = sw.part_len > 0 ? sw.part_len : ne.CB <= 128 ? kPartL / 2 : kPartL;
    const ChainPart cp = partition_chain(own_lo, own_hi - own_lo, sctrl(), close, part_len);
    n_own_sep = (int)cp.sep.size();
    pv.P = (int)cp.i0.size(); pv.s3 = 3 * sctrl();
    pv.q_off = 0; pv.m = n_own_sep;
    if (shard) {
      pv.m = 0;
      for (int r = 0; r < ts.world; ++r) {
        const ChainPart o = partition_chain(0, ts.cuts[r + 1] - ts.cuts[r], sctrl(), r + 1 < ts.world, part_len);
        if (r == ts.rank) pv.q_off = pv.m;
        pv.m += (int)o.sep.size();
      }
    }
    std::vector<int> tab, hb;                         // (pageable sources of asynchronous copies: they live until the synchronisation below)
    upload_partition(cp, tab);
    if (nbound > 0) {                                 // a time shard's halo tables
      if (ts.rank > 0) hb.push_back(ts.cuts[ts.rank]);
      if (ts.rank + 1 < ts.world) hb.push_back(ts.cuts[ts.rank + 1]);
      if (ts.rank > 0) hb.push_back(ts.rank - 1);
      if (ts.rank + 1 < ts.world) hb.push_back(ts.rank);
      halo_tables = own.template device<int>(hb.size());
      MVUS_HIP(hipMemcpyAsync(halo_tables, hb.data(), hb.size() * sizeof(int), hipMemcpyHostToDevice, be.stream));
    }
    MVUS_HIP(hipStreamSynchronize(be.stream));
    pv.VW = own.alloc((size_t)pv.P * kPartRowsMax * 2 * pv.s3);
  }
  void upload_partition(const ChainPart& cp, std::vector<int>& tab) {
    const auto& ts = be.tshard;
    const bool ghost = shard && ts.rank > 0;          // the separator that closes the previous rank's chain: left of interior 0
    std::vector<int> sl(pv.P, -1), sr(pv.P, -1), tc0, tpl, tpr, tgq, town;
    for (int k = 0; k < pv.P; ++k) {
      if (k < n_own_sep) sr[k] = cp.sep[k];
      if (k > 0) sl[k] = cp.sep[k - 1];
    }
    if (ghost) {
      sl[0] = 3 * (own_lo - sctrl());
      tc0.push_back(sl[0]); tpl.push_back(-1); tpr.push_back(0); tgq.push_back(pv.q_off - 1); town.push_back(0);
    }
    for (int k = 0; k < n_own_sep; ++k) {
      tc0.push_back(cp.sep[k]); tpl.push_back(k); tpr.push_back(k + 1 < pv.P ? k + 1 : -1); tgq.push_back(pv.q_off + k); town.push_back(1);
    }
    pv.nt = (int)tc0.size();
    for (const std::vector<int>* v : std::initializer_list<const std::vector<int>*>{&cp.i0, &cp.i1, &sl, &sr, &tc0, &tpl, &tpr, &tgq, &town}) tab.insert(tab.end(), v->begin(), v->end());
    const size_t seprow_at = tab.size();
    std::vector<unsigned char> srow((size_t)(ne.N3 + 3) / 4 * 4, 0);      // 1 = the row belongs to a separator (bytes, packed into the int table)
    for (int k = 0; k < n_own_sep; ++k) for (int a = 0; a < pv.s3; ++a) { const int r = cp.sep[k] + a; if (r >= 0 && r < ne.N3) srow[(size_t)r] = 1; }     // (rows as the tasks' tc0: local to the slice)
    tab.resize(tab.size() + srow.size() / 4);
    std::memcpy(tab.data() + seprow_at, srow.data(), srow.size());
    tab.push_back(0);
    int* part_tables = own.template device<int>(tab.size());
    MVUS_HIP(hipMemcpyAsync(part_tables, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, be.stream));
    pv.i0 = part_tables; pv.i1 = pv.i0 + pv.P; pv.sl = pv.i1 + pv.P; pv.sr = pv.sl + pv.P;
    pv.tc0 = pv.sr + pv.P; pv.tpl = pv.tc0 + pv.nt; pv.tpr = pv.tpl + pv.nt; pv.tgq = pv.tpr + pv.nt; pv.town = pv.tgq + pv.nt;
    pv.seprow = reinterpret_cast<const unsigned char*>(part_tables + seprow_at); pv.CB = ne.CB; pv.B = ne.B; pv.N3 = ne.N3; pv.Dl = nullptr; pv.direct = 0;
    pv.Et = ne.Et; pv.gs = ne.gs;
    pv_ready = true;
  }
  // the separator system: correction rows or back-correction, its buffers, cyclic reduction or the sequential kernels
  void plan_separators() {
    // One rank: the interiors' columns of Z are NOT corrected for the separators after the separator solve (k_part_back: a
    // read-modify-write of all of Z, 20 us at configs[2], 41 at configs[3]).  Block elimination gives
    //   E^T C^-1 E = E_I^T (B^-1 E_I) + R_S^T X_S,   R_S = E_S - H_SI B^-1 E_I  (the separators' reduced right-hand sides),
    // so the Schur product may pair the cross block with the UNCORRECTED interior solutions if the separators contribute R_S^T X_S: their
    // rows of Z are written as ZEROS by the right-hand-side copy (nothing from the main K range), R_S is kept beside the in-place solve
    // (pv.Dl) and R_S^T X_S runs as further rows of the product's K range over the compact arrays pv.Dl, pv.R (dealt to the same
    // wavefronts: schur_gemm_tile).  The step's own back-substitution is corrected for ONE vector (k_back_correct).  Time shards keep the back-correction: their separator sums run over the ranks.
    ncorr = 0;
    if (!wide && pv.m > 0 && !sw.part_back) {      // (round 6: time shards too -- R_S is the SUMMED reduced right-hand side there, copied beside the in-place solve after the ranks' sum)
      ncorr = 1;
      pv.Dl = own.alloc((size_t)pv.m * pv.s3 * ne.CB);
      // ... and the right-hand-side copy (Z = row-major E: a pass over both, the longer half of k_cholesky_and_rhs at configs[3]) is not
      // made at all: the interior solves' forward pass reads the assembled blocks (part_solve_block).  Z's separator rows are then
      // written by nobody: zeroed once, here.  (configs[3] 1.245 -> 1.218 ms, configs[2] 0.468 -> 0.460, configs[1] level.)
      pv.direct = sw.direct_rhs;
      if (pv.direct) MVUS_HIP(hipMemsetAsync(Z, 0, (size_t)ne.N3 * ncols * sizeof(double), be.stream));
    }
    const size_t mm = (size_t)std::max(pv.m, 1), ss = (size_t)pv.s3 * pv.s3;
    sep_count = mm * (2 * ss + (size_t)pv.s3 * ncols);
    sepbuf = own.alloc(sep_count);                    // [T | U | R]: one sum over the ranks
    pv.T = sepbuf; pv.U = pv.T + mm * ss; pv.R = pv.U + mm * ss;
    pv.U2 = own.alloc(mm * ss);
    pv.Ha = own.alloc(mm * ss);
    pv.Hc = own.alloc(mm * ss);
    bcr = bcr_plan(pv.m, pv.s3);
    use_bcr = bcr.lds <= 64 * 1024 && !sw.sep_sequential;
    bcr_done = own.template device<unsigned>(mm);
    MVUS_HIP(hipMemsetAsync(bcr_done, 0, mm * sizeof(unsigned), be.stream));
  }
  // time shards: the local separators eliminated by this rank alone, the world - 1 cut separators summed (MVUS_SEP_TWO_LEVEL=0: one level)
  void plan_two_level() {
    two_level = shard && use_bcr && !wide && sw.sep_two_level;
    if (!two_level) return;
    const auto& ts = be.tshard;
    const size_t ss = (size_t)pv.s3 * pv.s3;
    has_ghost = ts.rank > 0; has_cut = ts.rank + 1 < ts.world; ncut = ts.world - 1;
    k_loc = n_own_sep - has_cut;
    const size_t nc2 = (size_t)ncols + 2 * pv.s3;
    Rloc = own.alloc((size_t)std::max(k_loc, 1) * pv.s3 * nc2);
    CGK = own.alloc(2 * ss);
    cut_count = (size_t)ncut * (2 * ss + (size_t)pv.s3 * ncols);
    cutbuf = own.alloc(cut_count);
    cutws = own.alloc(3 * (size_t)std::max(ncut, 1) * ss);
    bcr_loc = bcr_plan(k_loc, pv.s3);
    bcr_cut = bcr_plan(ncut, pv.s3);
  }
  // Window-major assembly: needs every camera's frames in non-decreasing order (HostProblem::frames_sorted; anything else keeps the
  // detection-major kernel with its atomics).  Window length: about one wavefront of detections per (window, camera) -- the
  // Wn + 3 spans that reach a window hold (Wn + 3) * M / (C * N) detections on average -- within [4, 16] control points.
  bool win_usable() const {
    const HostProblem& hp = be.hp;
    if (!(hp.frames_sorted && hp.M > 0 && ne.N > 0 && hp.C <= 64 * kWinWaves && !sw.asm_atomic)) return false;
    // (the kernel keeps absolute detection indices in 32 bits and a camera's range length in 24: k_assemble_windows, cam_range)
    if (hp.M >= (int64_t)1 << 31) return false;
    for (int c = 0; c < hp.C; ++c) if (hp.det_off[c + 1] - hp.det_off[c] >= (1 << 24)) return false;
    return true;
  }
  // Window length AND camera groups, from one cost model.  A (window, camera) pair costs its batches of 64 staged detections -- (Wn + 3)
  // spans reach a window, so camera c brings n_c = (Wn + 3) rho_c + 3 of them, rho_c = detections per knot span -- a fixed part per
  // batch (evaluation, matrix-core pass) and a part per detection (accumulation); a workgroup walks the cameras of its group (C / G of
  // them, dealt over its four wavefronts) and pays a prologue of its own (the window's spline records); the grid of nwin x G workgroups
  // runs two per CU at a time.  Short windows repeat more evaluations (the three spans below a window) but fill the machine; camera
  // groups (round 6) fill it when the windows alone cannot -- a time shard's slice, few control points -- as long as a wavefront still
  // walks more than one camera.  MVUS_WIN / MVUS_WIN_GROUPS override.
  void win_plan() {
    const HostProblem& hp = be.hp;
    int Wn = 8, G = 1;
    int ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, be.device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    const double slots = 2.0 * ncu;
    const double nspan = shard ? std::max(1, own_hi - own_lo) : std::max(1, hp.N);      // control points the held detections spread over
    auto wg_cost = [&](int w) {
      double wg = 0.0;
      for (int c = 0; c < hp.C; ++c) {
        const double nc = (w + 3) * (double)(hp.det_off[c + 1] - hp.det_off[c]) / nspan + 3.0;
        wg += 0.45 * std::ceil(nc / 64.0) + 0.55 * nc / 64.0 + 0.15;      // + the camera's own set-up and stores
      }
      return wg;
    };
    // one group: the model of round 4 (measured optima 10 / 3 / 8 / 3 at configs[2] / [1] / [3] / [4], picks within 6 %)
    double best = 1e300;
    for (int w = 3; w <= kWinMaxW; ++w) {
      const double t = std::max(1.0, std::ceil((double)ne.N / w) / slots) * wg_cost(w);
      if (t < best * 0.999) { best = t; Wn = w; }
    }
    // camera groups only where that choice leaves a quarter or more of the workgroup slots empty, and only in ONE round of workgroups
    // (measured, `tools/micro/win_group_sweep.sh`: with the slots full, groups + longer windows are level at configs[2] -- 95-97 us against
    // 91-93 -- and the model cannot tell 13 x 4 (114 us) from 21 x 4 (97 us) there)
    if (std::ceil((double)ne.N / Wn) <= 0.75 * slots) {
      double bt = wg_cost(Wn) + 0.5;
      for (int g = 2; g <= 4; g *= 2) {
        if (hp.C <= kWinWaves * (g / 2)) break;
        for (int w = 3; w <= kWinMaxW; ++w) {
          if (std::ceil((double)ne.N / w) * g > 1.03 * slots) continue;      // (a handful of late workgroups is no second round)
          const double t = wg_cost(w) / g + 0.5;
          if (t < bt * 0.999) { bt = t; Wn = w; G = g; }
        }
      }
    }
    wv.Wn = sw.win > 0 ? std::min(kWinMaxW, sw.win) : Wn;
    wv.G = sw.win_groups > 0 ? std::min(8, sw.win_groups) : G;
    wv.nwin = (ne.N + wv.Wn - 1) / wv.Wn; wv.Ntot = hp.N;
  }
  // cameras dealt to the four wavefronts of a window by decreasing detection count, back and forth (0 1 2 3 3 2 1 0 ...): every
  // wavefront walks about the same number of detections whatever the cameras' frame rates
  std::vector<int32_t> win_camera_order() const {
    const HostProblem& hp = be.hp;
    std::vector<int32_t> perm((size_t)hp.C), byc((size_t)hp.C);
    for (int c = 0; c < hp.C; ++c) byc[c] = c;
    std::stable_sort(byc.begin(), byc.end(), [&](int32_t u, int32_t v) { return hp.det_off[u + 1] - hp.det_off[u] > hp.det_off[v + 1] - hp.det_off[v]; });
    const int ns = kWinWaves * wv.G;                       // wavefront slots that share the cameras of a window (G workgroups of four)
    std::vector<std::vector<int32_t>> of(ns);
    for (int i = 0; i < hp.C; ++i) { const int r = i % (2 * ns); of[r < ns ? r : 2 * ns - 1 - r].push_back(byc[i]); }
    // slot u walks perm[u], perm[u + ns], ...: it takes ceil((C - u) / ns) cameras, the first slots one more than the last ones
    std::vector<int32_t> flat;
    for (int v = 0; v < ns; ++v) flat.insert(flat.end(), of[v].begin(), of[v].end());
    std::vector<size_t> take(ns);
    for (int v = 0; v < ns; ++v) take[v] = v < hp.C ? (size_t)(hp.C - v + ns - 1) / ns : 0;
    size_t pos = 0;
    for (int v = 0; v < ns; ++v) for (size_t i = 0; i < take[v]; ++i) perm[(size_t)v + ns * i] = flat[pos++];
    return perm;
  }
  // per control point: where its spline starts in x, the spline's length, its knots, its place in the spline
  std::vector<int4> win_ctrl_records() const {
    const HostProblem& hp = be.hp;
    std::vector<int4> crec((size_t)std::max(1, hp.N), int4{0, 0, 0, 0});
    for (int sI = 0; sI < hp.S; ++sI) {
      const int ns = hp.ctrl_off[sI + 1] - hp.ctrl_off[sI];
      for (int jj = 0; jj < ns; ++jj)        // span l = jj + 3: knots t[l-2 .. l+3] start at knot_off + jj + 1
        crec[(size_t)hp.ctrl_off[sI] + jj] = int4{hp.xoff[sI] + jj, ns, hp.knot_off[sI] + jj + 1, (jj == 0 ? 1 : 0) | (jj + 4 == ns ? 2 : 0) | (jj + 4 > ns ? 4 : 0)};
    }
    return crec;
  }
  void win_prepare() {
    const HostProblem& hp = be.hp;
    use_win = win_usable();
    if (!use_win) return;
    win_plan();
    if (sw.debug) std::fprintf(stderr, "window-major assembly: %d control points per window, %d windows x %d camera group(s)\n", wv.Wn, wv.nwin, wv.G);
    wv.band_part = wv.G > 1 ? own.alloc((size_t)wv.G * ne.N * (3 + ne.W * 9)) : nullptr;
    const size_t psz = (size_t)(ne.B + 1) * (ne.B + 2) / 2;
    wv.Apart = own.alloc((size_t)wv.nwin * ne.C * psz);
    // six tables in one allocation: [cw | tlo | thi | flut | crec | cam_perm]
    const size_t bytes_cw = sizeof(CamWin) * (size_t)hp.C, bytes_t = sizeof(double) * ((size_t)hp.N + 1), bytes_l = sizeof(int32_t) * (((size_t)hp.flut_len + 3) & ~(size_t)3);
    const size_t bytes_r = sizeof(int4) * (size_t)std::max(1, hp.N), bytes_p = sizeof(int32_t) * (size_t)hp.C;
    Bump at;
    const size_t o_cw = at.take(bytes_cw), o_tlo = at.take(bytes_t), o_thi = at.take(bytes_t), o_flut = at.take(bytes_l), o_crec = at.take(bytes_r), o_perm = at.take(bytes_p);
    char* base = own.template device<char>(at.at);
    const std::vector<int32_t> perm = win_camera_order();
    const std::vector<int4> crec = win_ctrl_records();
    // (pageable sources: synchronised below, before perm and crec go)
    MVUS_HIP(hipMemcpyAsync(base + o_cw, hp.cam_win.data(), bytes_cw, hipMemcpyHostToDevice, be.stream));
    MVUS_HIP(hipMemcpyAsync(base + o_tlo, hp.win_tlo.data(), bytes_t, hipMemcpyHostToDevice, be.stream));
    MVUS_HIP(hipMemcpyAsync(base + o_thi, hp.win_thi.data(), bytes_t, hipMemcpyHostToDevice, be.stream));
    MVUS_HIP(hipMemcpyAsync(base + o_crec, crec.data(), bytes_r, hipMemcpyHostToDevice, be.stream));
    MVUS_HIP(hipMemcpyAsync(base + o_perm, perm.data(), bytes_p, hipMemcpyHostToDevice, be.stream));
    wv.cw = reinterpret_cast<const CamWin*>(base + o_cw);
    wv.tlo = reinterpret_cast<const double*>(base + o_tlo);
    wv.thi = reinterpret_cast<const double*>(base + o_thi);
    int32_t* flut = reinterpret_cast<int32_t*>(base + o_flut);
    wv.flut = flut;
    wv.crec = reinterpret_cast<const int4*>(base + o_crec);
    wv.cam_perm = reinterpret_cast<const int32_t*>(base + o_perm);
    hipLaunchKernelGGL(k_frame_lut, dim3((unsigned)((hp.flut_len + 255) / 256)), dim3(256), 0, be.stream, be.dp, wv.cw, flut, (long long)hp.flut_len);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipStreamSynchronize(be.stream));
    win_lds = (size_t)win_lds_doubles(ne.B) * sizeof(double);
    with_flag(hp.calib, [&](auto calib) { MVUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_assemble_windows<calib() ? 18 : 9>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)win_lds)); });
  }
  // the robust instantiation's dynamic LDS limit: set when a loss is first used on the handle (a handle without a loss does at
  // construction exactly what it always did)
  bool win_robust_ready = false;
  void win_robust_prepare() {
    if (win_robust_ready) return;
    with_flag(be.hp.calib, [&](auto calib) { MVUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_assemble_windows<calib() ? 18 : 9, true, LossSpec>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)win_lds)); });
    win_robust_ready = true;
  }

  // ---- two sets of blocks ----
  bool pv_ready = false;
  void bind_ne(int k) {
    NE = NEset[k];
    ne.A = NE; ne.gc = NE + off_gc; ne.Cb = NE + off_Cb; ne.gs = NE + off_gs; ne.Et = NE + off_Et; ne.Apart = NE + off_Apart;
    if (pv_ready) { pv.Et = ne.Et; pv.gs = ne.gs; }
    if (shard) { D = NE + nAg + halo_count; gx = D + be.hp.n; }      // (a time shard's diag(H) and g ride inside the summed head of the set)
  }
  // Speculative linearisation (ba_schur.h, launch_trial): one rank, the fused window-major assembly (every entry written by one plain
  // store: the second set needs no clearing), scalars fetched behind an event.  MVUS_NO_SPEC=1 keeps the sequential form for an A/B.
  // Time shards (round 6): the speculative assembly carries its collective with it -- every rank takes the same decision from the same
  // summed scalars, so every rank enqueues the same sequence; the scalars' copy to the host is enqueued in front of it (fetch_enqueue).
  bool spec_ok(int jac_mode) {
    if (!use_win || jac_mode != MVUS_JAC_ANALYTIC) return false;
    if (shard ? !be.spec_on_shards() : !be.scal_direct()) return false;
    if (sw.no_spec || sw.lm_materialize_j) return false;
    if (!NEset[1]) NEset[1] = own.alloc(ne_count + n_apart);
    return true;
  }
  void linearize_spec(BE&, const double* x_dev, double* f_dev, int jac_mode) {
    const bool pending = diag_pending;      // D and g in x order belong to the set the solver reads: untouched until adopt_spec
    // where the fetch that follows stops waiting: the start of the assembly kernel (a word in mapped memory), else an event in front of it
    if (!be.fetch_poll_begin(&wv.mark, &wv.mark_val)) { wv.mark = nullptr; be.fetch_mark(); }
    bind_ne(ne_cur ^ 1);
    linearize(be, x_dev, f_dev, jac_mode, true);
    bind_ne(ne_cur);
    wv.mark = nullptr;
    diag_pending = pending;
  }
  void adopt_spec() { ne_cur ^= 1; bind_ne(ne_cur); diag_pending = !shard; }
  // a rejected trial's speculative assembly may have raised the "row left the slice" flag for a point nobody keeps: forget it (a flag
  // raised by the CURRENT point's assembly has been acted on before any trial)
  void drop_spec() { if (shard) MVUS_HIP(hipMemsetAsync(fail + 1, 0, sizeof(int), be.stream)); }

  // x_fused != nullptr: the detection rows' Jacobian is evaluated inside the assembly kernel at x_fused (no J in memory);
  // the motion rows (O(T), tiny) still go through k_motion
  // the storage the assembly adds into; the LM driver has it zeroed beside its first residual evaluation (mark_cleared)
  bool ne_cleared = false;
  double* clear_ptr() { return use_win ? nullptr : NE; }      // (the window-major assembly writes every entry: nothing to clear)
  int64_t clear_len() const { return (int64_t)(ne_count + n_apart); }
  void mark_cleared() { ne_cleared = true; }
  bool last_atomic = false;                                // the last assembly went through the detection-major kernel (fp64 atomics)
  void motion_rows(const double* f_dev) {
    // (one rank: the row-ordered kernel in both modes -- 22 us against 26 for the LDS-window one at configs[1], and one source of
    // run-to-run differences less; a time shard keeps k_assemble_motion, which also reports rows that leave the slice)
    if (be.hp.T <= 0) return;
    const double* fm = f_dev + 2 * be.hp.M;
    const LossSpec loss = be.loss;
    if (wide) {
      const dim3 g((unsigned)ne.N), b(64);
      if (be.robust()) hipLaunchKernelGGL(k_det_motion_wide<true>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne, loss);
      else hipLaunchKernelGGL(k_det_motion_wide<false>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne);
    } else if (!shard && ne.W <= kDetMotW) {
      const dim3 g((unsigned)((ne.N + kThreads / 64 - 1) / (kThreads / 64))), b(kThreads);
      if (be.robust()) hipLaunchKernelGGL(k_det_motion<true>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne, loss);
      else hipLaunchKernelGGL(k_det_motion<false>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne);
    } else {
      const dim3 g((be.hp.T + kThreads - 1) / kThreads), b(kThreads);
      if (be.robust()) hipLaunchKernelGGL(k_assemble_motion<true>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne, loss);
      else hipLaunchKernelGGL(k_assemble_motion<false>, g, b, 0, be.stream, be.dp, be.mJ, be.mctrl, fm, ne);
    }
  }
  void assemble_local(const double* f_dev, const double* x_fused = nullptr, const int32_t* span_held = nullptr) {
    if (x_fused && use_win) {
      // window-major: every entry of A, gc, Cb, gs, Et is written by exactly one thread -- no clearing pass, no atomics.
      // It starts from the knot span of every detection at x: left behind by the residual evaluation at x that precedes every
      // linearisation (else evaluated now), or the held analytic Jacobian's own table
      ne_cleared = false; last_atomic = false;
      // (a time shard: the part of the packed head that is SUMMED over the ranks without being written in full here -- the halo exchange
      // buffer of the other ranks' cuts, diag(H) and g of the columns outside this slice -- starts from zero: ~1 MB, not the 36 MB of blocks)
      double* const zr = shard ? NE + nAg : (double*)nullptr;               // (cleared by k_cam_block_sum below: no launch of its own)
      const long long zn = shard ? (long long)(halo_count + 2 * (size_t)be.hp.n) : 0;
      if (span_held) wv.span = span_held;
      else {
        if (be.rspan_for != x_fused) be.residual(x_fused, const_cast<double*>(f_dev));      // (f_dev holds f(x) already: the same values again)
        wv.span = be.rspan;
      }
      be.ensure_cams(x_fused);
      if (be.robust()) win_robust_prepare();
      with_flag(be.hp.calib, [&](auto calib) {
        constexpr int B = calib() ? 18 : 9;
        const unsigned sumg = (unsigned)be.hp.C + (wv.G > 1 ? (unsigned)(((long long)ne.N * (3 + ne.W * 9) + 1023) / 1024) : 0u);
        if (be.robust()) hipLaunchKernelGGL((k_assemble_windows<B, true>), dim3(wv.nwin * wv.G), dim3(kWinThreads), win_lds, be.stream, be.dp, ne, wv, be.cams, x_fused, be.loss);
        else hipLaunchKernelGGL((k_assemble_windows<B, false>), dim3(wv.nwin * wv.G), dim3(kWinThreads), win_lds, be.stream, be.dp, ne, wv, be.cams, x_fused);
        hipLaunchKernelGGL(k_cam_block_sum<B>, dim3(sumg), dim3(1024), 0, be.stream, be.hp.C, wv.nwin, wv.Apart, ne, wv.G, (const double*)wv.band_part, zr, zn);
      });
      motion_rows(f_dev);
      MVUS_HIP(hipGetLastError());
      return;
    }
    if (!ne_cleared) be.fill(NE, 0.0, (int64_t)(ne_count + n_apart));      // one launch (hipMemsetAsync splits 36 MB into two fill kernels)
    ne_cleared = false;
    last_atomic = be.dp.n_chunks > 0;
    if (be.dp.n_chunks > 0) {
      const int nc = be.dp.n_chunks;
      const dim3 g(kGaParts * nc), b(kGaThreads);
      if (x_fused) be.ensure_cams(x_fused);
      // fused: the Jacobian is evaluated in the kernel at x_fused (no J, no span table); else the held blocks (no x)
      const double* Jh = x_fused ? nullptr : be.J;
      const int32_t* sh = x_fused ? nullptr : be.span;
      with_flag(be.hp.calib, [&](auto calib) {
        constexpr int NS = calib() ? 30 : 21;
        with_flag(x_fused != nullptr, [&](auto fused) {
          if (be.robust()) hipLaunchKernelGGL((k_assemble_spans<NS, fused(), true>), g, b, 0, be.stream, be.dp, Jh, sh, f_dev, ne, be.cams, x_fused, be.loss);
          else hipLaunchKernelGGL((k_assemble_spans<NS, fused(), false>), g, b, 0, be.stream, be.dp, Jh, sh, f_dev, ne, be.cams, x_fused);
        });
      });
    }
    if (be.dp.n_chunks > 0)
      with_flag(be.hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_cam_block_reduce<calib() ? 18 : 9>, dim3(be.hp.C, 2), dim3(1024), 0, be.stream, be.dp, ne); });
    motion_rows(f_dev);
    MVUS_HIP(hipGetLastError());
  }
  // Linearise at x: residual f (unless the caller already holds f(x) in f_dev), Jacobian, normal equations.  With the
  // analytic Jacobian the detection rows are fused (assemble_local above); other Jacobian modes materialise J first.
  void linearize(BE&, const double* x_dev, double* f_dev, int jac_mode, bool f_valid) {
    RoctxRange range("mvus linearise");
    const bool fused = jac_mode == MVUS_JAC_ANALYTIC && !sw.lm_materialize_j;
    if (!fused) { be.jacobian(x_dev, f_dev, jac_mode); assemble(be, f_dev); return; }
    if (!f_valid) be.residual(x_dev, f_dev);
    if (be.hp.T > 0) be.motion_jacobian(x_dev, f_dev);
    be.has_jacobian = false;                               // no materialised J belongs to this point
    assemble(be, f_dev, x_dev);
  }
  void assemble(BE&, const double* f_dev, const double* x_fused = nullptr, const int32_t* span_held = nullptr) {
    assemble_local(f_dev, x_fused, span_held);
    // mvus_ba_set_position_priors: the priors' rows are added behind every assembly, whatever produced the Jacobian -- at the point the fused
    // kernel linearised, else the one the stored Jacobian was evaluated at; a handle without active priors launches nothing here
    if (be.prior_active > 0) be.prior_normal_equations(ne, x_fused ? x_fused : be.jac_x);
    // mvus_ba_set_landmarks: the same on the camera side (A, gc), in front of the freeze pass, so held parameters stay held
    if (be.lm_active > 0) be.landmark_normal_equations(ne, x_fused ? x_fused : be.jac_x);
    // mvus_ba_set_frozen: every assembly -- window-major, detection-major, robust, the speculative one (the bound set is the one just
    // written) -- is followed by the freeze pass; a handle without a mask launches nothing here
    if (be.frozen_count > 0) {
      hipLaunchKernelGGL(k_freeze_ne, dim3((unsigned)be.frozen_count), dim3(kFreezeThreads), 0, be.stream, ne, (const int32_t*)be.frozen_idx, be.frozen_count);
      MVUS_HIP(hipGetLastError());
    }
    if (shard) {
      // time shard: sum the camera blocks and the blocks of the control points near a cut; the cross block never moves
      // ... and diag(H), g in x order: every rank adds its PARTIAL sums (rows of a control point near a cut sit on two
      // ranks), so they go into the same all-reduce, before the halo blocks are completed
      double* hb = NE + nAg;
      const int halo = be.tshard.halo;
      hipLaunchKernelGGL(k_halo_copy, dim3(256), dim3(256), 0, be.stream, ne, halo, nbound, halo_tables, halo_tables + nbound, Ntot, hb, 0, be.dp, D, gx, (long long)be.hp.n);
      be.reduce(NE, nAg + halo_count + 2 * (size_t)be.hp.n);
      hipLaunchKernelGGL(k_halo_copy, dim3(256), dim3(256), 0, be.stream, ne, halo, nbound, halo_tables, halo_tables + nbound, Ntot, hb, 1, be.dp, D, gx, (long long)be.hp.n);
    } else {
      be.reduce(NE, ne_count);          // observation shards: one sum-all-reduce of the packed normal-equation blocks per iteration
      diag_pending = true;              // D and g (x order) are written by the next solve's first kernel, or by flush_diag()
    }
    MVUS_HIP(hipGetLastError());
  }

  // normal equations of the Jacobian the backend holds: the analytic Jacobian of x_cur goes through the fused window-major assembly
  // (the LM path's kernel; MVUS_NE_FROM_J=1 forms them from the stored blocks instead), anything else is assembled from J
  // Under a mask or position priors the blocks the call before this one left here are used again, with the missing passes on top, where
  // the handle's memory says they may be (HandleMemory::blocks_reusable, ba_held.h; which entry points keep them: the table of ba_api.hip)
  // -- the masked system is then the raw blocks with the freeze pass applied, the difference between the exported blocks with and without
  // priors the priors' contribution, entry for entry, also behind the detection-major kernel, whose atomics would give a second assembly
  // other last bits.  A handle with neither a mask nor active priors assembles on every call, as always.
  void assemble_held(BE&) {
    const bool fused = be.held_analytic_at_xcur && use_win && !sw.ne_from_j;
    const BlocksTag want{be.frozen_count > 0, fused, be.prior_active > 0 ? be.prior_gen : 0, be.lm_active > 0 ? be.lm_gen : 0};
    if (be.mem.blocks_reusable(want)) {
      const BlocksTag& held = be.mem.held_blocks();
      if (held.prior_gen == 0 && want.prior_gen != 0) {
        be.prior_normal_equations(ne, fused ? be.x_cur : be.jac_x);
        diag_pending = true;
      }
      // (the landmarks' pass writes A and gc, which the freeze pass fixes -- unlike the priors', which stays on the spline side: where it goes
      // on top of blocks that are frozen already, the freeze pass, idempotent, runs again behind it)
      const bool landmarks_on_top = held.landmark_gen == 0 && want.landmark_gen != 0;
      if (landmarks_on_top) {
        be.landmark_normal_equations(ne, fused ? be.x_cur : be.jac_x);
        diag_pending = true;
      }
      if (want.frozen && (!held.frozen || landmarks_on_top)) {
        hipLaunchKernelGGL(k_freeze_ne, dim3((unsigned)be.frozen_count), dim3(kFreezeThreads), 0, be.stream, ne, (const int32_t*)be.frozen_idx, be.frozen_count);
        MVUS_HIP(hipGetLastError());
        diag_pending = true;
      }
    } else assemble(be, be.f_cur, fused ? be.x_cur : nullptr, fused ? be.span : nullptr);
    be.mem.stamp_blocks(want);
  }

  void flush_diag() {
    if (!diag_pending) return;
    const int tot = ne.CB + ne.N3;
    hipLaunchKernelGGL(k_ne_diag_grad, dim3((tot + 255) / 256), dim3(256), 0, be.stream, be.dp, ne, 0, D, gx);
    diag_pending = false;
  }
  // valid once the stream reaches this point: written by the solve that follows an assembly, or flushed here when none has run
  const double* grad_ptr() { flush_diag(); return gx; }
  const double* diag_ptr() { flush_diag(); return D; }
  const double* step_ptr() const { return px; }
  const int* fail_ptr() const { return fail; }
  bool solve_ok() const {                 // valid after the stream has been synchronised (the driver's fetch)
    if (shard) { fail_host[0] = fail_sum_code(be.scal_host[be.kFailSumSlot]); fail_host[1] = fail_sum_flag(be.scal_host[be.kFailSumSlot + 1]); }
    if (fail_host[1] & 2) throw HipError{"fused assembly: the span table does not belong to the point being linearised (internal error)"};
    if (fail_host[1] != 0) {
      be.reshard_flag = true;        // (the LM driver hands the point it has reached back to the caller: MVUS_E_RESHARD)
      throw HipError{"time shard: a detection or motion row reaches control points outside this rank's slice +- halo (the time stamps have drifted since the cuts were made): re-cut at the returned point", MVUS_E_RESHARD};
    }
    if (fail_host[0] != 0 && sw.debug) std::fprintf(stderr, "schur solve: fail code %d\n", fail_host[0]);
    return fail_host[0] == 0;
  }
  // A failed solve that is NOT a numerical failure: a workgroup of k_rcs_factor gave up waiting for the factor workgroup's hand-over
  // flag (a GPU shared with other processes or streams may not schedule workgroup 0 of a launch before the others: forward progress
  // between the workgroups of one launch is assumed there, not guaranteed).  The handle then takes the separate-launch route for the
  // rows below a super-block (MVUS_RCS_TRSM=launch: bit-identical results, no spinning) for the rest of its life and the caller
  // repeats the solve at the SAME damping -- raising lambda, the answer to a lost pivot, would silently change the iterates.
  bool retry_same() {
    if (fail_host[0] != kFailHandover || (rcs_trsm_launch && !bcr_fused)) return false;
    rcs_trsm_launch = true; bcr_fused = false;
    if (sw.debug) std::fprintf(stderr, "schur solve: hand-over time-out in k_rcs_factor / k_sep_bcr_levels -> a launch per stage from now on\n");
    return true;
  }

  // ---- cyclic reduction of a chain of separators (PartView v: its m nodes): wide levels, one-workgroup tail, right-hand sides ----
  template <int S3T> int bcr_levels(const PartView& v, int h) {      // a launch per level while it has more survivors than the tail takes; returns the tail's first stride
    for (; h <= v.m && v.m / (2 * h) > kBcrTailNs; h <<= 1)
      hipLaunchKernelGGL(k_sep_bcr_level<S3T>, dim3(v.m / (2 * h)), dim3(64), 0, be.stream, v, h, fail);
    return h;
  }
  template <int S3T> void bcr_tail(const PartView& v, int h) {
    if (h <= v.m) hipLaunchKernelGGL(k_sep_bcr_tail<S3T>, dim3(1), dim3(bcr_tail_waves(S3T) * 64), 0, be.stream, v, h, fail);
  }
  template <int S3T> void bcr_rhs(const PartView& v, int nc, const BcrPlan& plan) {
    if (plan.cols == kBcrCols) hipLaunchKernelGGL((k_sep_bcr_rhs<S3T, kBcrCols>), dim3((nc + kBcrCols - 1) / kBcrCols), dim3(256), plan.lds, be.stream, v, nc);
    else hipLaunchKernelGGL((k_sep_bcr_rhs<S3T, 1>), dim3(nc), dim3(256), plan.lds, be.stream, v, nc);
  }
  template <int S3T> void bcr_solve(const PartView& v, int nc, const BcrPlan& plan) {
    bcr_tail<S3T>(v, bcr_levels<S3T>(v, 1));
    bcr_rhs<S3T>(v, nc, plan);
  }
  template <int S3T> void sep_sequential(const PartView& v) {      // the block-tridiagonal kernels: chains too long for the cyclic reduction's LDS
    hipLaunchKernelGGL(k_sep_factor<S3T>, dim3(1), dim3(64), 0, be.stream, v, fail);
    hipLaunchKernelGGL(k_sep_rhs<S3T>, dim3((ncols + 63) / 64), dim3(64), 0, be.stream, v, ncols);
  }
  // one rank: ALL wide levels in one launch (k_sep_bcr_levels) where there are two to four of them; returns the stride reached (1: none run)
  template <int S3T> int bcr_fused_levels() {
    BcrLevels lv{};
    int total = 0, hh = 1;
    for (; hh <= pv.m && pv.m / (2 * hh) > kBcrTailNs && lv.nlev < 4; hh <<= 1) { lv.first[lv.nlev] = total; lv.h[lv.nlev] = hh; total += pv.m / (2 * hh); ++lv.nlev; }
    if (!(bcr_fused && !shard && lv.nlev >= 2 && !(hh <= pv.m && pv.m / (2 * hh) > kBcrTailNs))) return 1;
    bcr_epoch += 8;
    hipLaunchKernelGGL(k_sep_bcr_levels<S3T>, dim3(total), dim3(64), 0, be.stream, pv, lv, bcr_done, bcr_epoch, rcs_spin_limit, fail);
    return hh;
  }

  // time shards, round 6: the local separators are eliminated by this rank alone; only the world - 1 cut separators are summed (k_sep2_*)
  template <int S3T> void sep_two_level() {
    const int q0 = pv.q_off, cq0 = q0 - has_ghost, cqn = n_own_sep + has_ghost;
    // (no back-correction: the correction rows of the Schur product need this rank's parts of the reduced right-hand sides R_S as
    // they are before the solve overwrites them)
    const int nc2 = ncols + 2 * S3T;
    const size_t ssz = (size_t)S3T * S3T;
    double *CG = CGK, *CK = CGK + ssz;
    const long long nb = std::max((long long)k_loc * S3T * nc2 + 2 * S3T * S3T, ncorr > 0 ? (long long)cqn * S3T * ne.CB : 0LL);
    hipLaunchKernelGGL(k_sep2_build<S3T>, dim3((unsigned)std::min<long long>(2048, (nb + 255) / 256)), dim3(256), 0, be.stream, pv, q0, k_loc, has_ghost, has_cut, ncols, Rloc, CG, CK,
                       cq0, ncorr > 0 ? cqn * S3T : 0, ne.CB);
    if (k_loc > 0) {
      PartView pl = pv;                  // the local chain: nodes q0 .. q0 + k - 1 of the global arrays, renumbered from 0
      pl.m = k_loc; pl.T = pv.T + q0 * ssz; pl.U = pv.U + q0 * ssz; pl.U2 = pv.U2 + q0 * ssz; pl.Ha = pv.Ha + q0 * ssz; pl.Hc = pv.Hc + q0 * ssz; pl.R = Rloc;
      bcr_solve<S3T>(pl, nc2, bcr_loc);
    }
    hipLaunchKernelGGL(k_sep2_reduce<S3T>, dim3((unsigned)((cut_count + 255) / 256)), dim3(256), 0, be.stream, pv, q0, k_loc, has_ghost, has_cut,
                       be.tshard.rank, ncut, ncols, (const double*)Rloc, (const double*)CG, (const double*)CK, cutbuf);
    be.reduce(cutbuf, cut_count);        // every rank now holds the cut system
    PartView pc = pv;
    pc.m = ncut; pc.T = cutbuf; pc.U = cutbuf + ncut * ssz; pc.R = cutbuf + 2 * ncut * ssz;
    pc.U2 = cutws; pc.Ha = cutws + ncut * ssz; pc.Hc = cutws + 2 * ncut * ssz;
    // (the cyclic reduction again, not the sequential block-tridiagonal kernels: 7 nodes are three levels in one workgroup -- 63 us of
    // k_sep_factor + k_sep_rhs measured at world 8, configs[3], against ~25; so few nodes have no wide level: the tail alone)
    if (ncut > 2 * kBcrTailNs + 1) sep_sequential<S3T>(pc);      // (more than 33 ranks: the general kernels)
    else bcr_solve<S3T>(pc, ncols, bcr_cut);
    const long long tot = (long long)(k_loc + 2) * S3T * ncols;
    hipLaunchKernelGGL(k_sep2_finish<S3T>, dim3((unsigned)std::min<long long>(2048, (tot + 255) / 256)), dim3(256), 0, be.stream, pv, q0, k_loc, has_ghost, has_cut,
                       be.tshard.rank, ncut, ncols, (const double*)Rloc, (const double*)cutbuf);
  }
  // one rank, or every rank of a one-level time shard after the sum: the whole separator system
  template <int BWT, int S3T> void sep_one_level(bool split) {
    if (shard) {
      be.reduce(sepbuf, sep_count);        // every rank now holds the whole separator system
      // (no back-correction: the Schur product needs the reduced right-hand sides R_S as they are BEFORE the in-place solve -- on one rank
      // part_reduce_rhs writes them to pv.Dl as it forms them, here they exist only after the sum)
      if (ncorr > 0) MVUS_HIP(hipMemcpy2DAsync(pv.Dl, (size_t)ne.CB * sizeof(double), pv.R, (size_t)ncols * sizeof(double), (size_t)ne.CB * sizeof(double),
                                               (size_t)pv.m * pv.s3, hipMemcpyDeviceToDevice, be.stream));
    }
    if (!use_bcr) return sep_sequential<S3T>(pv);
    const int h = bcr_levels<S3T>(pv, bcr_fused_levels<S3T>());      // wide levels: one launch for all of them (or a launch each); the rest in one workgroup
    if (split) {                                                     // the tail beside the separators' right-hand sides
      const int tb = bcr_tail_waves(S3T) * 64, ny = (pv.s3 * ncols + tb - 1) / tb;
      hipLaunchKernelGGL((k_bcr_tail_and_reduce_rhs<BWT, S3T>), dim3(1 + pv.nt * ny), dim3(tb), 0, be.stream, pv, h, (int)(h <= pv.m), fail, ncols, Lb, Z, ny);
    } else bcr_tail<S3T>(pv, h);
    bcr_rhs<S3T>(pv, ncols, bcr);
  }

  // the partitioned band solver: interiors factorised and solved, the separators' system, (time shards) the interiors corrected
  template <int BWT, int S3T>
  void band_chain() {
    const dim3 gsolve(pv.P, (ncols + 63) / 64 + 1);      // + one block row for the coupling columns
    if (overlap_chol && !pv.direct) {
      const int cb = (pv.P + 7) / 8 * 8;
      hipLaunchKernelGGL(k_cholesky_and_rhs<BWT>, dim3((unsigned)(cb + xcd_grid(rhs_tiles_z))), dim3(256), 0, be.stream, pv, Lb, fail, cb, ne, ncols, Z, rhs_tiles_z, pv.Dl ? pv.seprow : (const unsigned char*)nullptr);
    } else hipLaunchKernelGGL(k_part_cholesky<BWT>, dim3(pv.P), dim3(64), 0, be.stream, pv, Lb, fail);
    hipLaunchKernelGGL(k_part_solve<BWT>, dim3(xcd_grid(pv.P * (int)gsolve.y)), dim3(64), 0, be.stream, pv, ncols, Lb, Z, (int)gsolve.y);
    if (pv.m <= 0) return;
    // other ranks' separators: zero here (one level: the whole system is summed; two levels: k_part_reduce writes every block this rank reads)
    if (shard && !two_level) MVUS_HIP(hipMemsetAsync(sepbuf, 0, sep_count * sizeof(double), be.stream));
    // one rank, cyclic reduction: only the matrix blocks first; the right-hand sides ride beside the one-workgroup tail
    const bool split = overlap_chol && !shard && use_bcr && pv.nt > 0;
    if (pv.nt > 0) hipLaunchKernelGGL(k_part_reduce<BWT>, dim3(pv.nt, split ? 1 : (pv.s3 * ncols + 255) / 256), dim3(256), 0, be.stream, pv, ncols, Lb, Z, split ? 1 : 3);
    if (shard && two_level) sep_two_level<S3T>();
    else sep_one_level<BWT, S3T>(split);
    if (ncorr == 0) {                                   // (one rank: no back-correction -- see where ncorr is set)
      const int gy = (ncols + 63) / 64, gz = (kPartRowsMax + kBackRows - 1) / kBackRows;
      const dim3 gback(xcd_grid(pv.P * gy * gz));
      hipLaunchKernelGGL(k_part_back<S3T>, gback, dim3(64), 0, be.stream, pv, ncols, Z, gy, gz);
    }
  }

  // time shards: the failure flags of a solve are SUMMED with the step (px[n], px[n + 1]); the LM driver's trial kernel forwards the sums
  // to the scalars its fetch brings to the host (trial_follows), any other caller gets them by a copy to the same two slots
  bool fail_in_scalars() const { return shard; }
  const double* fail_sum_ptr() const { return shard ? px + be.hp.n : (const double*)nullptr; }
  // ---- the stages of a solve, in order ----
  // damped band into Lb (and D, g in x order if an assembly left them pending); without the overlap also the right-hand sides Z = [E | gs]
  void pack_band(double lambda) {
    const long long nLb = (long long)ne.N3 * (BW + 1);
    const long long nZ = (long long)ne.N3 * ncols;          // >= nLb: one launch covers both passes
    const int rhs_tiles = (int)((std::max(nZ, nLb) + 255) / 256);
    if (overlap_chol) {
      const long long nband = std::max<long long>(nLb, (long long)ne.CB + ne.N3);
      hipLaunchKernelGGL(k_band_pack, dim3((unsigned)((nband + 255) / 256)), dim3(256), 0, be.stream, ne, lambda, BW, Lb, fail, be.dp, (int)diag_pending, D, gx);
      rhs_tiles_z = (int)((nZ + 255) / 256);
    } else {
      hipLaunchKernelGGL(k_build_rhs, dim3((unsigned)xcd_grid(rhs_tiles)), dim3(256), 0, be.stream, ne, ncols, Z, (!wide && pv.Dl) ? pv.seprow : (const unsigned char*)nullptr, lambda, BW, Lb, fail, be.dp,
                         (int)diag_pending, D, gx, rhs_tiles);
    }
    diag_pending = false;
  }
  void band_generic() {      // a band wider than six control points: one CU
    hipLaunchKernelGGL(k_band_chol_generic, dim3(1), dim3(256), (size_t)(BW + 1) * (BW + 1) * sizeof(double), be.stream, ne.N3, BW, Lb, fail);
    hipLaunchKernelGGL(k_band_solve_generic, dim3((unsigned)((ncols + 63) / 64)), dim3(64), (size_t)(BW + 1) * 64 * sizeof(double), be.stream, ne.N3, BW, ncols, Lb, Z);
  }
  // G = E Z over the owned rows, in nslab partial sums
  void schur_product() {
    const bool corr = !wide && ncorr > 0;
    // the separators whose R_S^T X_S this rank adds: all of them, or -- time shard -- its own (global numbers q_off ...)
    // (two levels: plus the ghost -- the cut separator's correction term splits into the two neighbours' own parts of R_S)
    const int cq0 = shard ? pv.q_off - (two_level ? has_ghost : 0) : 0, cqn = shard ? n_own_sep + (two_level ? has_ghost : 0) : pv.m;
    hipLaunchKernelGGL(k_schur_gemm, dim3(gemm_grid(ne.CB, nslab)), dim3(256), 0, be.stream, ne, ncols, 3 * own_lo, 3 * own_hi, nslab, ne.Et, Z, G,
                       corr ? (const double*)(pv.Dl + (size_t)cq0 * pv.s3 * ne.CB) : (const double*)nullptr, (const double*)(pv.R + (size_t)cq0 * pv.s3 * ncols),
                       corr ? cqn * pv.s3 : 0);
  }
  // time shards: the slabs summed into G0, then over the ranks; returns true when G0 holds the one sum the reduced camera system reads
  bool sum_ranks() {
    if (!shard) return false;
    const long long cnt = (long long)ne.CB * ncols;
    hipLaunchKernelGGL(k_sum_slabs, dim3((unsigned)((std::max<long long>(cnt, be.hp.n) + 255) / 256)), dim3(256), 0, be.stream, cnt, nslab, G, G0, px, (long long)be.hp.n);
    be.reduce(G0, (size_t)cnt);                   // the Schur complement contributions of all time slices
    return true;
  }
  // blocked L D L^T in block-image form (ba_rcs.hip.h): per super-panel of 144 unknowns one factor launch (one workgroup, the pivot
  // chain inside one CU), the rows below, the trailing blocks; one descending substitution at the end
  void rcs_ldlt(double lambda, const double* Gsum, int nsl) {
    const int nbk = rcs.nbk, nt = (16 * nbk + 31) / 32;
    hipLaunchKernelGGL(k_rcs_finish, dim3(nt, nt + 1), dim3(256), 0, be.stream, ne, ncols, nsl, lambda, Gsum, rcs, rcs_flags);
    for (int c0 = 0; c0 < nbk; c0 += kRcsSP) {
      const int nc = std::min(kRcsSP, nbk - c0), c1 = c0 + nc, m = nbk - c1;
      // (the block rows below the super-block are solved by m more workgroups of the same launch, one step behind the chain;
      // MVUS_RCS_TRSM=launch: by a launch of their own, for A/B)
      const bool fused_rows = m > 0 && !rcs_trsm_launch;
      hipLaunchKernelGGL(k_rcs_factor, dim3(1 + (fused_rows ? m : 0)), dim3(kRcsFactorThreads), 0, be.stream, rcs, c0, fail, (int)(m == 0), pc, rcs_flags, rcs_spin_limit);
      if (m > 0) {
        if (!fused_rows) hipLaunchKernelGGL(k_rcs_trsm, dim3(m), dim3(64 * kRcsTrsmWaves), (rcs_stage_doubles(nc) + 512) * sizeof(double), be.stream, rcs, c0);
        hipLaunchKernelGGL(k_rcs_syrk, dim3((m * (m + 1) / 2 + m + 3) / 4), dim3(256), 0, be.stream, rcs, c0);
      }
    }
    const int nsp = (nbk + kRcsSP - 1) / kRcsSP;                       // (the last super-panel is solved inside its factor launch)
    if (nsp > 1) hipLaunchKernelGGL(k_rcs_backsub, dim3(1), dim3(64 * kRcsBackWaves), rcs_backsub_doubles(nbk) * sizeof(double), be.stream, rcs, pc, nsp - 2);
  }
  // MVUS_RCS=gj: the block Gauss-Jordan of rounds 1-4 (A/B); the only reader of S, S2, Linv
  void rcs_gauss_jordan(double lambda, const double* Gsum, int nsl) {
    const int ntile = (ne.CB + kNB - 1) / kNB, nn = ne.CB;
    hipLaunchKernelGGL(k_schur_finish, dim3(ntile, ntile), dim3(kFinThreads), 0, be.stream, ne, ncols, nsl, lambda, Gsum, S, Linv, fail);
    double* a = S;
    double* b = S2;
    for (int kb = 0; kb < nn; kb += kNB) {
      const int nb = std::min(kNB, nn - kb), below = nn + 1 - (kb + nb);       // rows under the panel incl. the rhs row
      const bool last = kb + nb >= nn;
      hipLaunchKernelGGL(k_gj_step, dim3((below + kNB - 1) / kNB, (nn + kNB - 1) / kNB), dim3(kGjThreads), 0, be.stream, nn, kb, a, b, Linv, fail,
                         last ? pc : (double*)nullptr);
      std::swap(a, b);
    }
  }
  // p_s = -(z_g + Z_E p_c) over the owned rows, the one-vector correction for the separators, the ranks' parts of the step summed
  void back_substitute() {
    const int row_lo = 3 * own_lo, row_hi = 3 * own_hi, nrows = row_hi - row_lo, per = kThreads / 64;
    hipLaunchKernelGGL(k_back_substitute, dim3((unsigned)std::max(1, (nrows + per - 1) / per)), dim3(kThreads), 0, be.stream, be.dp, ne, ncols,
                       row_lo, row_hi, (int)(!shard || be.tshard.rank == 0), Z, pc, px, fail, (!shard && be.scal_direct()) ? fail_map : (int*)nullptr,
                       shard ? px + be.hp.n : (double*)nullptr);
    if (!wide && ncorr > 0) {                          // the interiors' rows were computed from uncorrected columns: one vector is corrected here
      if (BW == 11) hipLaunchKernelGGL(k_back_correct<9>, dim3(pv.P), dim3(256), 0, be.stream, be.dp, ne, pv, ncols, (const double*)pc, px);
      else hipLaunchKernelGGL(k_back_correct<15>, dim3(pv.P), dim3(256), 0, be.stream, be.dp, ne, pv, ncols, (const double*)pc, px);
    }
    if (shard) be.reduce(px, (size_t)be.hp.n + 2);             // every rank's part of the step (+ failure flags, packed by k_back_substitute)
    MVUS_HIP(hipGetLastError());
  }
  // the failure flags on their way to the host, where the solve did not write them into mapped memory
  void fetch_fail_flags(bool trial_follows) {
    if (shard) {
      if (!trial_follows) MVUS_HIP(hipMemcpyAsync(be.scal_host + be.kFailSumSlot, px + be.hp.n, 2 * sizeof(double), hipMemcpyDeviceToHost, be.stream));
    } else if (!be.scal_direct() || !fail_map) MVUS_HIP(hipMemcpyAsync(fail_host, fail, 2 * sizeof(int), hipMemcpyDeviceToHost, be.stream));
  }
  // READ-ONLY on the assembled blocks (A, gc, Cb, gs, Et of the bound set): everything a solve writes is its own workspace (Lb, Z, G, S,
  // the separator buffers, D / gx, px).  assemble_held relies on that -- a masked inspection call reuses the blocks an earlier call left
  // behind -- and so does a rejected trial, whose next solve reads the same blocks at another lambda.  Keep it so.
  void solve_async(double lambda, bool trial_follows = false) {
    RoctxRange range("mvus schur solve");
    pack_band(lambda);
    if (wide) band_generic();
    else if (BW == 11) band_chain<11, 9>();
    else band_chain<17, 15>();
    schur_product();
    const bool summed = sum_ranks();
    const double* Gsum = summed ? G0 : G;
    const int nsl = summed ? 1 : nslab;
    if (sw.rcs_gj) rcs_gauss_jordan(lambda, Gsum, nsl);
    else rcs_ldlt(lambda, Gsum, nsl);
    back_substitute();
    fetch_fail_flags(trial_follows);
  }
};

// Gauss-Newton normal equations of the Jacobian currently held, copied out for inspection (mvus_ba_normal_equations)
template <class BE>
int schur_export(BE& be, HipSchur<BE>& sc, double* g, double* JtJ_cam, double* band, double* cross, int32_t* W_out) {
  if (!be.has_jacobian) { be.err = "no Jacobian held: call mvus_ba_residual_jacobian first"; return MVUS_E_INVALID; }
  if (sc.shard) { be.err = "normal_equations: not available on a time shard (every rank holds a slice of the spline blocks)"; return MVUS_E_INVALID; }
  if (W_out) *W_out = sc.ne.W;
  if (!g && !JtJ_cam && !band && !cross) return MVUS_OK;
  sc.assemble_held(be);
  sc.flush_diag();
  const NEView& ne = sc.ne;
  if (g) be.download(g, sc.gx, be.hp.n);
  if (JtJ_cam) be.download(JtJ_cam, ne.A, (int64_t)ne.C * ne.B * ne.B);
  if (band) be.download(band, ne.Cb, (int64_t)ne.N * ne.W * 9);
  if (cross) {
    std::vector<double> Ec((size_t)ne.N3 * ne.CB);
    be.download(Ec.data(), ne.Et, (int64_t)Ec.size());
    for (int c = 0; c < ne.C; ++c)
      for (int r = 0; r < ne.N3; ++r)
        for (int k = 0; k < ne.B; ++k) cross[((size_t)c * ne.B + k) * ne.N3 + r] = Ec[((size_t)c * ne.N3 + r) * ne.B + k];
  }
  return MVUS_OK;
}

}  // namespace mvus
