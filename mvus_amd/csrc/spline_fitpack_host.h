// FITPACK's scalar routines that fppara's control flow runs on the host (fpdisc, fpknot, fprati), restated line by line.  No HIP.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace mvus {

// ---- host side of fppara ------------------------------------------------------------------------------------------------
namespace fitpack {

// fpdisc.f for k = 3 (k2 = 5): b[(n - 8) * 5], 0-based row l - k2 for l = k2..nk1
inline void fpdisc(const std::vector<double>& t, int n, std::vector<double>& b) {
  const int k2 = 5, k1 = 4, k = 3, nk1 = n - k1, nrint = nk1 - k;
  const double an = nrint, fac = an / (t[nk1] - t[k1 - 1]);
  b.assign((size_t)std::max(0, n - 2 * k1) * k2, 0.0);
  double h[8];
  for (int l = k2; l <= nk1; ++l) {
    const int lmk = l - k1;
    for (int j = 1; j <= k1; ++j) {
      const int ik = j + k1, lj = l + j, lk = lj - k2;
      h[j - 1] = t[l - 1] - t[lk - 1];
      h[ik - 1] = t[l - 1] - t[lj - 1];
    }
    int lp = lmk;
    for (int j = 1; j <= k2; ++j) {
      int jk = j;
      double prod = h[j - 1];
      for (int i = 1; i <= k; ++i) { jk = jk + 1; prod = prod * h[jk - 1] * fac; }
      const int lk = lp + k1;
      b[(size_t)(lmk - 1) * k2 + (j - 1)] = (t[lk - 1] - t[lp - 1]) / prod;
      lp = lp + 1;
    }
  }
}

// fpknot.f: one more knot, in the interval with the largest residual that still holds samples (1-based bookkeeping kept)
inline void fpknot(const double* x, std::vector<double>& t, int& n, std::vector<double>& fpint, std::vector<int>& nrdata, int& nrint) {
  const int k = (n - nrint - 1) / 2;
  double fpmax = 0.0;
  int jbegin = 1, number = 0, maxpt = 0, maxbeg = 0;
  for (int j = 1; j <= nrint; ++j) {
    const int jpoint = nrdata[j - 1];
    if (!(fpmax >= fpint[j - 1] || jpoint == 0)) { fpmax = fpint[j - 1]; number = j; maxpt = jpoint; maxbeg = jbegin; }
    jbegin = jbegin + jpoint + 1;
  }
  const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, next = number + 1;
  if (next <= nrint) {
    for (int j = next; j <= nrint; ++j) {
      const int jj = next + nrint - j;
      fpint[jj] = fpint[jj - 1];
      nrdata[jj] = nrdata[jj - 1];
      const int jk = jj + k;
      t[jk] = t[jk - 1];
    }
  }
  nrdata[number - 1] = ihalf - 1;
  nrdata[next - 1] = maxpt - ihalf;
  const double am = maxpt;
  double an = nrdata[number - 1];
  fpint[number - 1] = fpmax * an / am;
  an = nrdata[next - 1];
  fpint[next - 1] = fpmax * an / am;
  const int jk = next + k;
  t[jk - 1] = x[nrx - 1];
  n = n + 1;
  nrint = nrint + 1;
}

// `nplus` calls of fpknot (stopping like fppara when n reaches nmax or nest) with the same result in O(nrint + nplus log nrint):
// fpknot scans all intervals for the largest residual and shifts three arrays per knot -- O(n) each, 0.2 s of host time in a
// fit that ends with 25 000 knots.  Here the intervals are a linked list in time order and the candidates (intervals that
// still hold samples) a heap ordered like fpknot's scan: the largest fpint, the EARLIEST interval among equal ones (its scan
// replaces the maximum only by a strictly larger value).  In a state fpknot itself does not handle (no interval with a positive
// residual and samples left: it would index interval 0) the insertions stop.
inline void fpknot_batch(const double* x, std::vector<double>& t, int& n, std::vector<double>& fpint, std::vector<int>& nrdata, int& nrint, int nplus,
                         int nmax, int nest) {
  if (nplus <= 0) return;
  if (nplus < 8 || nrint < 64) {                     // few insertions: the plain calls
    for (int l = 0; l < nplus; ++l) { fpknot(x, t, n, fpint, nrdata, nrint); if (n == nmax || n == nest) break; }
    return;
  }
  const int k = (n - nrint - 1) / 2;
  struct Node { double fp, tright; int nr, jbegin, next, version; };
  std::vector<Node> nodes;
  nodes.reserve((size_t)nrint + (size_t)nplus);
  {
    int jbegin = 1;
    for (int j = 0; j < nrint; ++j) {
      nodes.push_back(Node{fpint[j], j + 1 < nrint ? t[k + 1 + j] : 0.0, nrdata[j], jbegin, j + 1 < nrint ? j + 1 : -1, 0});
      jbegin = jbegin + nrdata[j] + 1;
    }
  }
  struct Cand { double fp; int jbegin, node, version; };
  auto worse = [](const Cand& a, const Cand& b) { return a.fp < b.fp || (a.fp == b.fp && a.jbegin > b.jbegin); };      // heap top = max fp, then min jbegin
  std::vector<Cand> heap;
  heap.reserve((size_t)nrint + 2 * (size_t)nplus);
  for (int j = 0; j < nrint; ++j) if (nodes[j].nr != 0 && nodes[j].fp > 0.0) heap.push_back(Cand{nodes[j].fp, nodes[j].jbegin, j, 0});
  std::make_heap(heap.begin(), heap.end(), worse);
  int added = 0;
  bool fallback = false;
  for (int l = 0; l < nplus; ++l) {
    while (!heap.empty() && heap.front().version != nodes[heap.front().node].version) { std::pop_heap(heap.begin(), heap.end(), worse); heap.pop_back(); }
    if (heap.empty()) { fallback = true; break; }
    std::pop_heap(heap.begin(), heap.end(), worse);
    const Cand c = heap.back();
    heap.pop_back();
    Node& a = nodes[c.node];
    const double fpmax = a.fp;
    const int maxpt = a.nr, maxbeg = a.jbegin;
    const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf;
    Node b;
    b.tright = a.tright; b.next = a.next; b.version = 0;
    a.nr = ihalf - 1;
    b.nr = maxpt - ihalf;
    const double am = maxpt;
    double an = a.nr;
    a.fp = fpmax * an / am;
    an = b.nr;
    b.fp = fpmax * an / am;
    a.tright = x[nrx - 1];
    b.jbegin = nrx;                                   // = maxbeg + (ihalf - 1) + 1
    ++a.version;
    const int bi = (int)nodes.size();
    a.next = bi;
    const Cand ca{a.fp, a.jbegin, c.node, a.version}, cb{b.fp, b.jbegin, bi, 0};
    const bool push_a = a.nr != 0 && a.fp > 0.0, push_b = b.nr != 0 && b.fp > 0.0;
    nodes.push_back(b);                               // (invalidates a)
    if (push_a) { heap.push_back(ca); std::push_heap(heap.begin(), heap.end(), worse); }
    if (push_b) { heap.push_back(cb); std::push_heap(heap.begin(), heap.end(), worse); }
    ++added;
    if (n + added == nmax || n + added == nest) break;
  }
  // back to fpknot's arrays, in time order
  {
    const int nr2 = nrint + added;
    int j = 0;
    for (int i = 0; i != -1; i = nodes[i].next, ++j) {
      fpint[j] = nodes[i].fp;
      nrdata[j] = nodes[i].nr;
      if (nodes[i].next != -1) t[k + 1 + j] = nodes[i].tright;
    }
    // (like fpknot, nothing behind the interior knots is maintained: fppara rewrites the k + 1 end knots before every pass)
    n += added;
    nrint = nr2;
  }
  (void)fallback;
}

inline double fprati(double& p1, double& f1, double p2, double f2, double& p3, double& f3) {
  double p;
  if (p3 > 0.0) {
    const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
    p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
  } else {
    p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
  }
  if (f2 < 0.0) { p3 = p2; f3 = f2; } else { p1 = p2; f1 = f2; }
  return p;
}

}  // namespace fitpack
}  // namespace mvus
