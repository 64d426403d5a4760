"""The Schur product's tile decode, accumulator map and slab plan (mvus_amd/csrc/ba_gemm_plan.h), checked without a GPU by a stand-alone
host program (tests/hostcheck/gemm_plan_hostcheck.cpp) that this file builds with g++ and runs."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostcheck', 'gemm_plan_hostcheck.cpp')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_hostcheck')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-o', exe, SRC])
    return exe


def _plan(prog, CB, rows, cus, forced=0):
    out = subprocess.run([prog, 'plan', str(CB), str(rows), str(cus), str(forced)], check=True, capture_output=True, text=True).stdout
    nslab, on_xcd, grid = (int(v) for v in out.split())
    return nslab, on_xcd, grid


def test_every_tile_once_and_every_needed_sub_block_written_once(prog):
    """nbk = 1 ... 24 block rows, CB a multiple of 48 and ragged at the 48 and at the 16 level: the t -> (bi, bj) decode yields every tile
    of the block lower triangle exactly once; over all tiles every 16x16 sub-block on or below the diagonal and every 16-row piece of the
    right-hand-side column has exactly one writer, nothing above the diagonal is written, and the (hi, lo) rule of k_schur_finish /
    k_rcs_finish only ever points at a written sub-block."""
    r = subprocess.run([prog, 'cover'], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def test_slab_plan_at_the_benchmark_shape(prog):
    """CB = 288 (21 tiles), 15 009 rows, 256 CUs: three slabs per XCD fit the 64 workgroup slots (63), a fourth does not -- 24 slabs."""
    nslab, on_xcd, grid = _plan(prog, 288, 15009, 256)
    assert nslab == 24
    assert on_xcd == 63 and on_xcd <= 64
    assert grid == 8 * 21 * 3


@pytest.mark.parametrize('CB,rows,want', [
    (63, 3000, (47, 18, 144)),          # 3 tiles, 188 row sets: one set per wavefront, six slabs on an XCD
    (576, 24009, (32, 312, 2496)),      # 78 tiles: five rounds of an XCD's 64 slots at four slabs per XCD
])
def test_slab_plan_pinned(prog, CB, rows, want):
    """What the cost model gives with the tile count nbk (nbk + 1) / 2, 256 CUs: (slabs, workgroups on the busiest XCD, grid)."""
    assert _plan(prog, CB, rows, 256) == want


def test_forced_slab_count_is_taken_as_it_is(prog):
    assert _plan(prog, 288, 15009, 256, forced=11) == (11, 42, 336)
    assert _plan(prog, 153, 540, 256, forced=24)[0] == 24
