"""What a BA handle remembers from one API call to the next (mvus_amd/csrc/ba_held.h: HandleMemory), checked without a GPU: the record
itself through the hostcheck_mem_* entries, and the host build of the LM driver over the same record (hostcheck_lm_chain)."""
import ctypes
import itertools

import numpy as np
import pytest

from golden_util import load_case
from hostcheck_util import HostHandle, load
from mvus_amd import _lib
from mvus_amd import problem as mp

# the table's rows (ba_api.hip): (keeps carry, KeepBlocks: 0 none, 1 unfrozen, 2 all)
TRANSPARENT, KEEPS_BLOCKS, KEEPS_RAW_BLOCKS, KEEPS_NOTHING = (1, 2), (0, 2), (0, 1), (0, 0)
JAC = _lib.JAC_ANALYTIC


class Memory:
    """A bare HandleMemory."""

    def __init__(self):
        self.lib = load()
        self.m = ctypes.c_void_p(self.lib.hostcheck_mem_new())

    def __del__(self):
        self.lib.hostcheck_mem_free(self.m)

    def begin_call(self, row):
        self.lib.hostcheck_mem_begin_call(self.m, row[0], row[1])

    def resume(self, x, usable=True):
        return self.lib.hostcheck_mem_resume(self.m, _lib.dptr(x), x.size, int(usable))

    def remember(self, slot, x, mirror=None):
        self.lib.hostcheck_mem_remember(self.m, slot, _lib.dptr(x), x.size, _lib.dptr(mirror) if mirror is not None else None)

    def take_carry(self, jac_mode=JAC, usable=True):
        cost = ctypes.c_double(0)
        r = self.lib.hostcheck_mem_take_carry(self.m, jac_mode, int(usable), ctypes.byref(cost))
        return bool(r & 1), bool(r & 2), cost.value

    def keep_carry(self, lin_valid, cost=1.0, jac_mode=JAC):
        self.lib.hostcheck_mem_keep_carry(self.m, 1, int(lin_valid), cost, jac_mode)

    def damping(self, op=0, lam=0.0, nu=0.0):
        out = np.zeros(2)
        self.lib.hostcheck_mem_damping(self.m, op, lam, nu, _lib.dptr(out))
        return tuple(out)

    def reusable(self, frozen, fused=True, prior_gen=0):
        return bool(self.lib.hostcheck_mem_blocks(self.m, 0, int(frozen), int(fused), prior_gen))

    def stamp(self, frozen, fused=True, prior_gen=0):
        self.lib.hostcheck_mem_blocks(self.m, 1, int(frozen), int(fused), prior_gen)

    def forget(self):
        self.lib.hostcheck_mem_blocks(self.m, 2, 0, 0, 0)


# ---- the model check: the parent commit's rule, restated, against the record -------------------------------------------------------------

class ParentRule:
    """The rule as the parent commit had it, spread over HipBackend (api_seq, carry, carry_seq, lm_last), HipSchur (held_seq, held_frozen,
    carry_held) and the lines inside each entry point of ba_api.hip.  Every call is served (no early return)."""

    def __init__(self):
        self.api_seq = self.carry_seq = self.held_seq = 0
        self.carry = (False, False)            # f_valid, lin_valid
        self.armed = self.held_frozen = False

    def carry_held(self, keep_frozen=True):
        if self.held_seq != 0 and self.held_seq + 1 == self.api_seq and (keep_frozen or not self.held_frozen):
            self.held_seq = self.api_seq

    def solve(self, ok, lin):                  # from the point the last solve returned; ok: reaches lm_remember / lm_keep
        self.api_seq += 1
        resumed, self.armed = self.armed, False
        taken = (False, False)
        if resumed:                            # lm_carry
            if self.carry[0] and self.carry_seq + 1 == self.api_seq:
                taken = self.carry
            self.carry = (False, False)
        if ok:
            self.armed, self.carry, self.carry_seq = True, (True, lin), self.api_seq
        return resumed, taken

    def register(self):
        self.api_seq += 1
        if self.carry_seq + 1 == self.api_seq:
            self.carry_seq = self.api_seq
        self.carry_held()

    def set_position_priors(self):
        self.api_seq += 1
        self.carry = (False, False)
        self.carry_held()

    def set_frozen(self):
        self.api_seq += 1
        self.carry = (False, False)
        self.carry_held(False)

    def set_loss(self):
        self.api_seq += 1
        self.carry = (False, False)

    def residual(self):
        self.api_seq += 1

    def lm_step(self, masked):                 # assemble_held with frozen_count > 0 (masked) or not, no priors, one assembly route
        self.api_seq += 1
        self.carry_held()
        reuse = masked and self.held_seq == self.api_seq and (not self.held_frozen or masked)
        self.held_seq, self.held_frozen = self.api_seq, masked
        return reuse


class RecordRule:
    """The same calls over HandleMemory: begin_call with the entry's row, then what the entry itself asks of the record."""

    def __init__(self):
        self.mem = Memory()
        self.x = np.array([1.0, 2.0, 3.0])

    def solve(self, ok, lin):
        self.mem.begin_call(KEEPS_NOTHING)
        resumed = self.mem.resume(self.x) >= 0
        taken = self.mem.take_carry()[:2] if resumed else (False, False)
        if ok:
            self.mem.remember(0, self.x)
            self.mem.keep_carry(lin)
        return resumed, taken

    def register(self):
        self.mem.begin_call(TRANSPARENT)

    def set_position_priors(self):
        self.mem.begin_call(KEEPS_BLOCKS)

    def set_frozen(self):
        self.mem.begin_call(KEEPS_RAW_BLOCKS)

    def set_loss(self):
        self.mem.begin_call(KEEPS_NOTHING)

    residual = set_loss

    def lm_step(self, masked):
        self.mem.begin_call(KEEPS_BLOCKS)
        reuse = self.mem.reusable(masked)
        self.mem.stamp(masked)
        return reuse


ALPHABET = {
    'solve, blocks at x': lambda r: r.solve(True, True),
    'solve, blocks stale': lambda r: r.solve(True, False),
    'solve, refused': lambda r: r.solve(False, False),
    'register': lambda r: r.register(),
    'set_position_priors': lambda r: r.set_position_priors(),
    'set_frozen': lambda r: r.set_frozen(),
    'set_loss': lambda r: r.set_loss(),
    'residual': lambda r: r.residual(),
    'lm_step, masked': lambda r: r.lm_step(True),
    'lm_step, unmasked': lambda r: r.lm_step(False),
}
PROBES = ('solve, blocks at x', 'lm_step, masked')      # is the carry taken by the next solve (and with lin_valid)?  are the blocks reused by the next lm_step?


def test_the_record_decides_as_the_parent_rule_did_for_every_short_sequence():
    """Every sequence of up to four calls from ALPHABET, followed by each probe: each solve's (resumed, carry taken, with lin_valid) and each
    lm_step's reuse are those of the parent's rule -- in particular without the four explicit `carry = LmCarry{}` the parent had."""
    count = 0
    for length in range(5):
        for seq in itertools.product(ALPHABET, repeat=length):
            for probe in PROBES:
                old, new = ParentRule(), RecordRule()
                for name in seq + (probe,):
                    a, b = ALPHABET[name](old), ALPHABET[name](new)
                    assert a == b, (seq, probe, name, a, b)
                count += 1
    assert count == 2 * sum(len(ALPHABET) ** k for k in range(5))


def test_the_model_sees_every_decision_both_ways():
    """(the sweep above is not vacuous: carries taken with and without lin_valid and let lapse, blocks reused and not)"""
    r = ParentRule()
    assert r.solve(True, True) == (False, (False, False)) and r.solve(True, False) == (True, (True, True)) and r.solve(True, True) == (True, (True, False))
    r.residual()
    assert r.solve(True, True) == (True, (False, False))
    r.register()
    assert r.solve(True, True) == (True, (True, True))
    assert not r.lm_step(True) and r.lm_step(True) and not r.lm_step(False) and r.lm_step(True)
    r.set_frozen()
    assert not r.lm_step(True)


# ---- the record's parts ------------------------------------------------------------------------------------------------------------------

def test_resume_point():
    mem, x = Memory(), np.array([0.5, -0.0, np.nan, 4.0])
    assert mem.resume(x) == -1                                   # nothing remembered
    mem.remember(1, x)
    assert mem.resume(x) == 1 and mem.resume(x) == -1            # disarmed on consult
    mem.remember(0, x)
    y = x.copy()
    y[1] = 0.0                                                   # equal as numbers, not as bits; the NaN is equal as bits
    assert mem.resume(y) == -1 and mem.resume(x) == -1           # ... and a failed comparison disarms as well
    mem.remember(0, x)
    assert mem.resume(x, usable=False) == -1 and mem.resume(x) == -1
    mem.remember(-1, x)                                          # the point is in neither of the driver's buffers
    assert mem.resume(x) == -1
    # without a mirror the point is copied; a mirror is used where it lies
    z = x.copy()
    mem.remember(0, z)
    z[0] = 7.0
    assert mem.resume(x) == 0
    mirror = x.copy()
    mem.remember(1, x, mirror)
    mirror[3] = 5.0
    assert mem.resume(x) == -1
    mem.remember(1, x, mirror)
    assert mem.resume(mirror) == 1


def test_carry_is_for_the_next_call_only_and_for_its_jacobian_mode():
    mem = Memory()
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry() == (False, False, 0.0)
    mem.keep_carry(True, cost=2.5)
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry() == (True, True, 2.5) and mem.take_carry() == (False, False, 0.0)      # disarmed on consult
    mem.keep_carry(True, cost=2.5)
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry(jac_mode=_lib.JAC_PATTERN) == (True, False, 2.5)                         # f(x) holds, the blocks are another Jacobian's
    mem.keep_carry(True)
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry(usable=False) == (False, False, 0.0) and mem.take_carry() == (False, False, 0.0)
    mem.keep_carry(True, cost=3.0)
    mem.begin_call(TRANSPARENT)
    mem.begin_call(TRANSPARENT)
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry() == (True, True, 3.0)
    mem.keep_carry(True)
    mem.begin_call(TRANSPARENT)
    mem.begin_call(KEEPS_BLOCKS)
    mem.begin_call(TRANSPARENT)
    mem.begin_call(KEEPS_NOTHING)
    assert mem.take_carry() == (False, False, 0.0)


def test_damping_clamps_and_reset():
    mem = Memory()
    assert mem.damping() == (0.0, 0.0)
    assert mem.damping(1, 0.25, 8.0) == (0.25, 8.0)
    assert mem.damping(1, 1e-20, 2.0) == (1e-12, 2.0)
    assert mem.damping(1, 1e9, 4096.0) == (1e6, 1024.0)
    assert mem.damping() == (1e6, 1024.0)
    assert mem.damping(2) == (0.0, 0.0)


def test_blocks_token():
    mem = Memory()
    mem.begin_call(KEEPS_BLOCKS)
    assert not mem.reusable(True)                                # nothing stamped
    mem.stamp(False)
    assert mem.reusable(True) and not mem.reusable(False)        # raw blocks: the freeze pass goes on top; no mask, no priors: assembled anyway
    assert mem.reusable(False, prior_gen=3) and mem.reusable(True, prior_gen=3)
    assert not mem.reusable(True, fused=False)                   # the other assembly route's blocks
    mem.stamp(True, prior_gen=3)
    assert mem.reusable(True, prior_gen=3)
    assert not mem.reusable(True, prior_gen=4) and not mem.reusable(True) and not mem.reusable(False, prior_gen=3)      # no pass comes off again
    mem.begin_call(KEEPS_RAW_BLOCKS)
    assert not mem.reusable(True, prior_gen=3)                   # frozen blocks are the old mask's
    mem.stamp(False, prior_gen=3)
    mem.begin_call(KEEPS_RAW_BLOCKS)
    assert mem.reusable(True, prior_gen=3)
    mem.begin_call(KEEPS_NOTHING)
    mem.begin_call(KEEPS_BLOCKS)
    assert not mem.reusable(True, prior_gen=3)                   # lapsed for good
    mem.stamp(False)
    mem.forget()
    assert not mem.reusable(True)
    mem.begin_call(KEEPS_BLOCKS)
    assert not mem.reusable(True)


# ---- the LM driver over the record: a chain of short solves, as bench.py's headline loop runs them ---------------------------------------

BUDGETS = [2, 2, 2, 3, 2, 2, 2, 3]


@pytest.fixture(scope='module')
def chains():
    scene, g = load_case('rs_F_2int_3cam')
    prob, _ = mp.problem_from_scene(scene)
    opts = _lib.default_opts(_lib.SOLVER_LM_SCHUR, JAC, 2)
    K = len(BUDGETS)

    def run(memory, rows=None, poison=None):
        return HostHandle(prob).lm_chain(g['x0'], opts, BUDGETS, memory, rows, poison)

    def row(r):
        return r[0] + 2 * r[1]

    return {'x0': np.asarray(g['x0'], dtype=np.float64), 'off': run(False), 'on': run(True),
            'plain': [run(True, [-1] + [row(r)] * (K - 1)) for r in (KEEPS_NOTHING, KEEPS_BLOCKS, KEEPS_RAW_BLOCKS)],
            'registration': run(True, [-1] + [row(TRANSPARENT)] * (K - 1)),
            'refused': [run(m, None, [0, 0, 1, 0, 0, 1, 0, 0]) for m in (False, True)]}


def same_results(a, b):
    return all(np.array_equal(p.x, q.x) and (p.cost, p.nfev, p.njev, p.status) == (q.cost, q.nfev, q.njev, q.status) for p, q in zip(a, b))


def evaluations(chain):
    return [(s.n_residual, s.n_jacobian) for s in chain]


def test_chain_memory_changes_when_work_is_done_never_a_value(chains):
    off = chains['off']
    assert off[-1].cost < off[0].cost and any(not np.array_equal(off[k].x, off[k + 1].x) for k in range(len(off) - 1))
    for other in [chains['on'], chains['registration']] + chains['plain']:
        assert same_results(off, other)


def test_chain_each_continued_solve_saves_what_the_last_left(chains):
    """One residual evaluation always (f at the returned point is there); one linearisation as well where the solve before ended with the
    blocks of the point it returned -- by convergence or with its last trial rejected -- and not where it ended on its budget with an
    accepted step (the host Schur has no speculative linearisation: the driver reports that as SolveResult::jac_stale).  Of the solves
    with one trial, the one that moved x ended the second way and the one that left x where it was the first."""
    off, on = chains['off'], chains['on']
    assert evaluations(on)[0] == evaluations(off)[0]
    for k in range(1, len(off)):
        prev = off[k - 1]
        if BUDGETS[k - 1] == 2 and prev.status == 0:
            moved = not np.array_equal(prev.x, off[k - 2].x if k >= 2 else chains['x0'])
            assert prev.jac_stale == moved
        saved = (off[k].n_residual - on[k].n_residual, off[k].n_jacobian - on[k].n_jacobian)
        assert saved == (1, 0 if prev.jac_stale else 1), (k, saved, prev.jac_stale)
    print('jac_stale per solve:', [s.jac_stale for s in off], 'evaluations off:', evaluations(off), 'on:', evaluations(on))


def test_chain_a_call_in_between_costs_the_carry_unless_it_is_transparent(chains):
    off, on = chains['off'], chains['on']
    for plain in chains['plain']:
        assert evaluations(plain) == evaluations(off)
    assert evaluations(chains['registration']) == evaluations(on)
    assert evaluations(on) != evaluations(off)


def test_chain_a_refused_solve_leaves_no_point_behind(chains):
    """A solve handed a NaN refuses after it has consulted the remembered point: the next solve, from the last good point, finds neither
    the point nor a carry and evaluates like one on a handle without memory; the one after continues as usual."""
    off, on = chains['refused']
    assert [s.status for s in off] == [s.status for s in on] and off[2].status == off[5].status == -3
    assert all(np.array_equal(p.x, q.x) for p, q in zip(off, on))
    assert np.array_equal(on[2].x, on[1].x) and np.array_equal(on[5].x, on[4].x)
    for k in (3, 6):
        assert evaluations(on)[k] == evaluations(off)[k]
    for k in (1, 4, 7):
        assert on[k].n_residual == off[k].n_residual - 1
