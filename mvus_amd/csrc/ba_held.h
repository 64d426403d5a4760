// HandleMemory: what a BA handle remembers from one API call to the next, and the one rule that times it.  Plain C++ (no HIP): the
// library's backend and the host test backend hold the same record (tests/test_handle_memory_host.py checks the rule without a GPU).
//
//   the point the last LM solve returned          resume / remember      (which of the driver's two x buffers holds it, and a host copy)
//   what that solve left valid at that point      take_carry / keep_carry (f(x), its cost, maybe the normal equations: LmCarry)
//   the damping                                   damping / store_damping / reset_damping
//   a token for the normal-equation blocks the    blocks_reusable / stamp_blocks / forget_blocks
//   previous call assembled under a mask or priors
//   the call counter                              begin_call
//
// Carry and blocks are valid for the NEXT call on the handle only.  Every entry point opens with begin_call(row); a row that keeps one of
// them moves its stamp on to this call, so that it is still "the previous call's" for the one after (the table of rows: ba_api.hip,
// DESIGN.md section 4.8).  What a row does not keep lapses by the counter alone -- nothing has to be cleared.
// Not here: the pointer-identity caches (cams_for, rspan_for), the bounds cache, the held-Jacobian flags: those follow buffers, not calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ba_solver.h"

namespace mvus {

enum class KeepBlocks { none, unfrozen, all };      // unfrozen: only blocks without a freeze pass on them (mvus_ba_set_frozen: frozen ones belong to the old mask)
struct CallKeeps { bool carry; KeepBlocks blocks; };
// what was applied to the blocks a call left: the freeze pass, the fused (window-major) or the from-J assembly, the priors' generation (0: none),
// the landmarks' generation (0: none)
struct BlocksTag { bool frozen = false, fused = false; uint64_t prior_gen = 0, landmark_gen = 0; };
struct LmDamping { double lambda = 0, nu = 0; };      // 0: where a fresh handle starts

struct HandleMemory {
  void begin_call(CallKeeps k) {
    ++seq;
    if (k.carry && carry_seq + 1 == seq) carry_seq = seq;
    const bool keep = k.blocks == KeepBlocks::all || (k.blocks == KeepBlocks::unfrozen && !held.frozen);
    if (keep && held_seq != 0 && held_seq + 1 == seq) held_seq = seq;
  }

  // ---- the point the last LM solve returned: slot 0 / 1 of the driver's two x buffers, -1 none ----
  // Consulting the remembered point DISARMS it: from here on the solve writes into both buffers (upload, trial points), so only a solve
  // that reaches remember -- a normal or a reshard exit -- re-arms it.  A solve that leaves early (non-finite cost at x0, an exception)
  // therefore cannot leave a stale "buffer k holds the point I returned" behind for a caller that retries from the last good point.
  int resume(const double* x_host, int64_t n, bool usable) {
    int r = -1;
    if (last >= 0 && last_ptr != nullptr && usable && std::memcmp(last_ptr, x_host, sizeof(double) * n) == 0) r = last;
    last = -1; last_ptr = nullptr;
    return r;
  }
  // mirror: a host buffer that holds the returned point already and stays as it is until the next solve has consulted the point (the
  // pinned mirror the accepted trial's kernel wrote: every solve starts its trials at mirror 0 again, but compares before it launches one);
  // nullptr -- a solve that accepted no step returns the caller's x -- copies the point
  void remember(int slot, const double* x_host, int64_t n, const double* mirror) {
    last = slot; last_ptr = nullptr;
    if (last < 0) return;
    if (mirror != nullptr) last_ptr = mirror;
    else { last_host.assign(x_host, x_host + n); last_ptr = last_host.data(); }
  }

  // ---- what the last LM solve left for that point (ba_schur.h).  Consulting it disarms it as well: a solve that fails early must not leave it behind ----
  LmCarry take_carry(int jac_mode, bool usable) {
    LmCarry c{};
    if (carry.f_valid && carry_seq + 1 == seq && usable) {
      c = carry;
      if (carry_jac_mode != jac_mode) c.lin_valid = false;
    }
    carry = LmCarry{};
    return c;
  }
  void keep_carry(const LmCarry& c, int jac_mode) { carry = c; carry_seq = seq; carry_jac_mode = jac_mode; }

  // ---- LM damping and its growth factor, from one solve on the handle to the next ----
  LmDamping damping() const { return damp; }
  void store_damping(double lambda, double nu) { damp = {std::min(std::max(lambda, 1e-12), 1e6), std::min(nu, 1024.0)}; }
  void reset_damping() { damp = {}; }      // another problem (loss, set of unknowns)

  // ---- the blocks of the held Jacobian, as the previous call left them in the Schur workspace ----
  // Under a mask or priors they are assembled ONCE: blocks the call before this one left (and every call since kept) are used again when
  // they differ from the wanted ones by passes that go ON TOP only -- the priors' pass where they carry none (never other priors), the landmarks' pass
  // where they carry none (never other landmarks; it writes the camera blocks, so on frozen blocks the caller runs the freeze pass again
  // behind it: HipSchur::assemble_held), the freeze pass where they are raw (never the other way).  Without a mask and without priors every call assembles, as always.
  bool blocks_of_this_call() const { return held_seq != 0 && held_seq == seq; }
  const BlocksTag& held_blocks() const { return held; }
  bool blocks_reusable(const BlocksTag& want) const {
    return (want.frozen || want.prior_gen != 0 || want.landmark_gen != 0) && blocks_of_this_call() && held.fused == want.fused &&
           (held.prior_gen == 0 || held.prior_gen == want.prior_gen) && (held.landmark_gen == 0 || held.landmark_gen == want.landmark_gen) &&
           (!held.frozen || want.frozen);
  }
  void stamp_blocks(const BlocksTag& tag) { held_seq = seq; held = tag; }
  void forget_blocks() { held_seq = 0; held = {}; }      // the workspace that held them is gone

 private:
  uint64_t seq = 0, carry_seq = 0, held_seq = 0;
  int last = -1;
  const double* last_ptr = nullptr;      // host copy of the remembered point: the caller's mirror (no copy), else last_host
  std::vector<double> last_host;
  LmCarry carry{};
  int carry_jac_mode = -1;
  LmDamping damp;
  BlocksTag held;
};

}  // namespace mvus
