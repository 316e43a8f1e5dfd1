"""The two block -> tile maps of csrc/metro_common.h, walked on the host (no GPU): block_stream_map, which conv_pw64.hip and
conv_pws.hip use to give each block its output-channel slab and its tile stream, and xcd_block_lid, which the ring kernel and the
tap-reuse 3x3 use to give each block its one tile.  Both are __host__ __device__ integer arithmetic on (block, grid), so the
code the kernels run is compiled for the host here (tests/helpers.py: compile_for_host) and checked for EVERY grid a device
could ask for -- the grid cap is CUs x resident blocks, so a partitioned device or a build with METRO_CU_LIMIT reaches grids
the MI355X of the GPU tests never launches:

  * for every grid 1 .. 4096 and halves in {1, 2, 4, 8} with halves | grid, block -> (half, first tile) is a bijection onto
    halves x G, G = grid / halves: every tile stream gets every slab once, no block works on another block's tiles;
  * wherever the XCD branch is taken (grid a multiple of 8, grid / 8 a multiple of halves) the `halves` blocks of one stream
    have the same block & 7: they sit on one XCD and share the stream's input tiles in its L2 (the point of the branch);
  * lid is a bijection onto [0, nblk) for every nblk 1 .. 4096.

The checks are held against two planted faults in a Python restatement of each map (as tests/test_crop_assignment.py plants
layout faults): `q` in place of `q + 1` in the lid map, and a dropped `/ halves` in the stream map.  The restatements themselves
are held to the compiled code at every point."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import compile_for_host

GRIDS = range(1, 4097)
HALVES = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    dll = compile_for_host(tmp_path_factory.mktemp('host_block_maps'), 'host_block_maps', ['metro_common.h'], '''
extern "C" void host_block_stream_map(int grid, int halves, int* half, int* first) {
    for (int b = 0; b < grid; ++b) {
        const metro::BlockStream s = metro::block_stream_map(b, grid, halves);
        half[b] = s.half; first[b] = s.first;
    }
}
extern "C" void host_xcd_block_lid(int nblk, int* lid) {
    for (int b = 0; b < nblk; ++b) lid[b] = metro::xcd_block_lid(b, nblk);
}
''')
    ip = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')
    dll.host_block_stream_map.argtypes, dll.host_block_stream_map.restype = [C.c_int, C.c_int, ip, ip], None
    dll.host_xcd_block_lid.argtypes, dll.host_xcd_block_lid.restype = [C.c_int, ip], None
    return dll


# ---- the maps restated (fault = None), and each with one planted fault ---------------------------------------------------
def stream_map_py(grid, halves, fault=None):
    b = np.arange(grid)
    if grid % 8 == 0 and (grid // 8) % halves == 0:
        xcd, j = b & 7, b >> 3
        per_xcd = grid // 8 if fault == 'dropped / halves' else grid // 8 // halves
        return j % halves, xcd * per_xcd + j // halves
    return b % halves, b // halves


def lid_map_py(nblk, fault=None):
    b = np.arange(nblk)
    q, r = nblk >> 3, nblk & 7
    q1 = q if fault == 'q for q + 1' else q + 1
    xcd, idx = b & 7, b >> 3
    return np.where(xcd < r, xcd * q1, r * q1 + (xcd - r) * q) + idx


# ---- the checks: None, or what is wrong ------------------------------------------------------------------------------------
def stream_map_faults(grid, halves, half, first):
    g = grid // halves
    if half.min() < 0 or half.max() >= halves or first.min() < 0 or first.max() >= g:
        return f'grid {grid}, halves {halves}: (half, first tile) outside [0, {halves}) x [0, {g})'
    if len(np.unique(first.astype(np.int64) * halves + half)) != grid:
        return f'grid {grid}, halves {halves}: two blocks share (half, first tile)'
    if grid % 8 == 0 and (grid // 8) % halves == 0:
        xcd = np.arange(grid) & 7
        order = np.argsort(first, kind='stable')
        if (xcd[order].reshape(g, halves) != xcd[order].reshape(g, halves)[:, :1]).any():
            return f'grid {grid}, halves {halves}: the blocks of one tile stream sit on different XCDs'
    return None


def lid_map_faults(nblk, lid):
    if not np.array_equal(np.sort(lid), np.arange(nblk)):
        return f'nblk {nblk}: lid is not a bijection onto [0, {nblk})'
    return None


def test_stream_map_is_a_bijection_and_keeps_a_stream_on_one_xcd(host):
    n_xcd = 0
    for halves in HALVES:
        for grid in GRIDS:
            if grid % halves:
                continue
            half, first = np.empty(grid, np.int32), np.empty(grid, np.int32)
            host.host_block_stream_map(grid, halves, half, first)
            ph, pf = stream_map_py(grid, halves)
            assert np.array_equal(half, ph) and np.array_equal(first, pf), f'grid {grid}, halves {halves}: the restatement differs'
            fault = stream_map_faults(grid, halves, half, first)
            assert fault is None, fault
            n_xcd += grid % 8 == 0 and (grid // 8) % halves == 0
    assert n_xcd >= 4096 // 8 + 4096 // 16 + 4096 // 32 + 4096 // 64       # the XCD branch was walked at every halves


def test_lid_map_is_a_bijection(host):
    for nblk in GRIDS:
        lid = np.empty(nblk, np.int32)
        host.host_xcd_block_lid(nblk, lid)
        assert np.array_equal(lid, lid_map_py(nblk)), f'nblk {nblk}: the restatement differs'
        fault = lid_map_faults(nblk, lid)
        assert fault is None, fault


def test_planted_faults_are_rejected():
    # q for q + 1: wrong wherever nblk & 7 != 0 and some XCD behind the first holds a block (nblk >= 2)
    for nblk in GRIDS:
        want_fault = nblk & 7 != 0 and nblk >= 2
        got = lid_map_faults(nblk, lid_map_py(nblk, 'q for q + 1'))
        assert (got is not None) == want_fault, (nblk, got)
    # a dropped / halves: wrong wherever the XCD branch is taken with halves > 1 and the grid has more than one block per XCD run
    for halves in HALVES:
        for grid in GRIDS:
            if grid % halves:
                continue
            xcd_branch = grid % 8 == 0 and (grid // 8) % halves == 0
            got = stream_map_faults(grid, halves, *stream_map_py(grid, halves, 'dropped / halves'))
            assert (got is not None) == (xcd_branch and halves > 1), (grid, halves, got)
    # and a stream spread over two XCDs (the plain map's order used on an XCD-branch grid) is seen by the XCD check alone
    b = np.arange(64)
    assert 'different XCDs' in stream_map_faults(64, 4, b % 4, b // 4)
