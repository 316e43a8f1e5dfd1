"""The kernel-level heat-map entries (metro_heat_marginals, metro_heat_modes, metro_heat_posterior) and the case lists of
tests/test_gpu_heat_volumes.py, without a GPU: the new C symbols and their refusals, the ids of their dry runs, the CPU half of
the workgroup cases (every case has, on the fp64 restatement alone, the property it claims, and stays within the cap on modes of
negligible mass), and a closure of the GPU cases over the shape classes the supported grid reaches.

The closure: for every head of the grid of tests/test_kernel_coverage.py (proc_side 64 .. 512 x stride 4 .. 32 x three heads,
depth 8) and every `precise`, the class each kernel takes there -- computed with the kernel files' own helpers, compiled for the
host (md_slab_rows, po_fits, hm_tile_pixels, hm_chunk_pixels) --

    modes        whole / slabs / refused; the last slab ragged or not
    posterior    staged / streamed
    marginals    tile 32 / 64; the last tile ragged or not; C over 256 or not; chunk below the tile or not

must be launched by a case of the GPU file at that `precise`.  The one class no case can launch is the modes' `refused`: it is held
by test_c_refusals (METRO_ERR_UNSUPPORTED at the smallest refused side of the grid)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests import heat_modes_ref as MR
from tests import test_gpu_heat_volumes as G
from tests import test_heat_marginals as TH, test_heat_modes as TM, test_heat_posterior as TP
from tests.helpers import compile_for_host
from tests.test_gpu_heat_marginals import HEAT_IDS
from tests.test_gpu_heat_modes import MODES_IDS
from tests.test_heat_posterior import POST_IDS
from tests.test_kernel_coverage import GRID_DATASETS, GRID_SIDES, GRID_STRIDES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('metro_heat_marginals_scratch_bytes', 'metro_heat_marginals', 'metro_heat_modes', 'metro_heat_posterior')
_DRY = C.c_void_p(4096)         # any aligned non-NULL pointer: a dry run launches nothing
OK, INVALID, UNSUPPORTED = 0, -1, -2
PRECISION_OF = {0: 'f16', 1: 'f32', 2: 'f64'}


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_in_header_bindings_library_and_heads(lib):
    raw = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    assert raw.index('int  metro_heat_marginals(') > raw.index('---- single-kernel entry points')
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1, name
        assert ('void* stream' in params) == (name != 'metro_heat_marginals_scratch_bytes'), name
    from metro_pose3d_amd import heads
    assert all(callable(getattr(heads, f)) for f in ('marginals_from_logits', 'modes_from_logits', 'posterior_from_logits'))
    assert 'metro_heat_marginals' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def dry(lib, fn, *args):
    """The status and the ids of one call in a dry run (metro_kernel_notes(2)): nothing is launched, whatever the status."""
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        st = fn(*args)
        return st, lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)


def entry_calls(lib, cs, precise=0, n=2, k=2, radius=1, logits=_DRY, scratch=_DRY, out=(_DRY, _DRY), prior=_DRY):
    """{kernel: (status, ids)} of the three entries on one set of arguments."""
    ref = C.byref(cs) if cs is not None else None
    return {'marginals': dry(lib, lib.metro_heat_marginals, logits, n, ref, precise, scratch, out[0], out[1], None),
            'modes': dry(lib, lib.metro_heat_modes, logits, n, ref, precise, k, radius, out[0], out[1], None),
            'posterior': dry(lib, lib.metro_heat_posterior, logits, n, ref, precise, prior, out[0], None)}


def test_dry_run_ids(lib):
    cs = G.make_spec(8, 17, 8, G.repeat_last(17))
    for precise, precision in PRECISION_OF.items():
        got = entry_calls(lib, cs, precise)
        assert got == {'marginals': (OK, HEAT_IDS[precision]), 'modes': (OK, MODES_IDS[precision]), 'posterior': (OK, POST_IDS[precision])}, got
    # the records alone, no copy of the logits: [n][tiles][C][2] and [n][J][2] doubles, each rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256
    assert lib.metro_heat_marginals_scratch_bytes(C.byref(cs), 3) == up(3 * 2 * 136 * 2 * 8) + up(3 * 17 * 2 * 8)


def test_c_refusals(lib):
    cs = G.make_spec(8, 17, 8, G.repeat_last(17))
    all_invalid = lambda got: all(st == INVALID and ids == '' for st, ids in got.values())
    assert all_invalid(entry_calls(lib, cs, logits=None)) and all_invalid(entry_calls(lib, None))
    assert all_invalid(entry_calls(lib, cs, out=(None, _DRY)))
    got = entry_calls(lib, cs, out=(_DRY, None))
    assert got['marginals'][0] == got['modes'][0] == INVALID and got['posterior'][0] == OK           # the posterior has one output
    assert entry_calls(lib, cs, scratch=None)['marginals'][0] == INVALID and entry_calls(lib, cs, prior=None)['posterior'][0] == INVALID
    # alignment: the logits to their element, the scratch to 16 bytes, every other pointer to 4
    assert all_invalid(entry_calls(lib, cs, logits=C.c_void_p(4098))) and all_invalid(entry_calls(lib, cs, precise=2, logits=C.c_void_p(4100)))
    assert all(st == OK for st, _ in entry_calls(lib, cs, precise=1, logits=C.c_void_p(4100)).values())
    assert all_invalid(entry_calls(lib, cs, out=(C.c_void_p(4098), _DRY)))
    assert entry_calls(lib, cs, scratch=C.c_void_p(4104))['marginals'][0] == INVALID
    assert entry_calls(lib, cs, prior=C.c_void_p(4097))['posterior'][0] == INVALID
    assert b'aligned' in lib.metro_last_error()
    for n in (0, -1, 65536):
        assert all_invalid(entry_calls(lib, cs, n=n)), n
        assert lib.metro_heat_marginals_scratch_bytes(C.byref(cs), n) == -1
    assert all(st == OK for st, _ in entry_calls(lib, cs, n=65535).values())
    assert lib.metro_heat_marginals_scratch_bytes(None, 1) == -1
    for k in (0, 9):
        assert entry_calls(lib, cs, k=k)['modes'] == (INVALID, '') and b'k %d outside' % k in lib.metro_last_error()
    for radius in (-1, 4):
        assert entry_calls(lib, cs, radius=radius)['modes'] == (INVALID, '') and b'radius %d outside' % radius in lib.metro_last_error()
    assert all(entry_calls(lib, cs, k=k, radius=r)['modes'][0] == OK for k, r in ((1, 0), (8, 3)))
    for precise in (3, -1):
        assert all_invalid(entry_calls(lib, cs, precise=precise)), precise
    # joint counts, depth, stride, side, permutation
    for field, bad in (('n_joints_head', 0), ('n_joints_head', 65), ('n_joints_out', 0), ('n_joints_out', 65), ('depth', 0), ('stride', 0),
                       ('proc_side', 31)):
        broken = G.make_spec(8, 17, 8, G.repeat_last(17))
        setattr(broken, field, bad)
        assert all_invalid(entry_calls(lib, broken)), (field, bad)
    broken = G.make_spec(8, 17, 8, G.repeat_last(17))
    broken.permutation[3] = 17
    assert all_invalid(entry_calls(lib, broken)) and b'permutation' in lib.metro_last_error()
    # shapes a kernel cannot serve: the modes' flags and three rows do not fit the LDS; the posterior's voxel index
    for side, precise, want in ((84, 0, OK), (88, 0, UNSUPPORTED), (88, 1, UNSUPPORTED), (72, 2, OK), (80, 2, UNSUPPORTED), (128, 0, UNSUPPORTED),
                                (2048, 0, UNSUPPORTED)):
        got = entry_calls(lib, G.make_spec(side, 17, 8, G.repeat_last(17)), precise, n=1)
        assert got['modes'][0] == want and (want == OK or got['modes'][1] == ''), (side, precise, got['modes'])
        assert G.modes_class(side, 8, precise) == ('refused',) if want else G.modes_class(side, 8, precise)[0] == 'slabs'
    lib.metro_heat_modes(_DRY, 1, C.byref(G.make_spec(88, 17, 8, G.repeat_last(17))), 0, 2, 1, _DRY, _DRY, None)
    assert b'does not fit' in lib.metro_last_error()
    assert entry_calls(lib, G.make_spec(1448, 17, 8, G.repeat_last(17)), n=1)['posterior'][0] == OK               # 16 773 632 voxels
    assert entry_calls(lib, G.make_spec(1449, 17, 8, G.repeat_last(17)), n=1)['posterior'] == (UNSUPPORTED, '')    # more than 2^24
    assert entry_calls(lib, G.make_spec(2048, 17, 8, G.repeat_last(17)), n=1)['posterior'] == (UNSUPPORTED, '')


def test_heads_helpers_check_their_arguments_without_a_launch():
    import torch
    from metro_pose3d_amd import heads
    spec = ModelSpec(50, 32, 'h36m')
    good = torch.zeros((2, 8, 8, spec.n_head_channels))
    for fn, extra in ((heads.marginals_from_logits, ()), (heads.modes_from_logits, ()),
                      (lambda lg, sp, **kw: heads.posterior_from_logits(lg, torch.zeros((2, 17, 9)), sp, **kw), ())):
        with pytest.raises(ValueError, match='logits must be'):
            fn(good[:, :7], spec)
        with pytest.raises(ValueError, match='precise must be'):
            fn(good, spec, precise=3)
    for kw in (dict(k=0), dict(k=9), dict(radius=-1), dict(radius=4), dict(k=True)):
        with pytest.raises(ValueError, match='must be an int in'):
            heads.modes_from_logits(good, spec, **kw)
    with pytest.raises(ValueError, match='prior must be'):
        heads.posterior_from_logits(good, torch.zeros((2, 16, 9)), spec)


# ---- the shape classes: the kernel files' own helpers ----------------------------------------------------------------------------

@pytest.fixture(scope='module')
def helpers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('host_heat_volumes')
    modes, post = TM.load_host(tmp), TP.load_host(tmp)
    marg = compile_for_host(tmp, 'host_heat_marginals', ['heat_marginals.hip'], TH.HOST_BODY)
    for fn, args in ((marg.host_tile_pixels, 1), (marg.host_chunk_pixels, 3)):
        fn.restype, fn.argtypes = C.c_int, [C.c_int] * args
    return modes, post, marg


def kernel_class(helpers, kernel, side, j, d, precise):
    """The class of one launch from the kernel file's helpers (the mirrors of the GPU file are held to these)."""
    modes, post, marg = helpers
    logit_bytes, acc_bytes = (8 if precise == 2 else 4), (4 if precise == 0 else 8)
    if kernel == 'modes':
        rows = modes.host_slab_rows(side, d, logit_bytes)
        assert rows == G.slab_rows(side, d, logit_bytes), (side, d, logit_bytes)
        got = ('refused',) if rows == 0 else ('whole',) if rows >= side else ('slabs', 'ragged' if side % rows else 'even')
    elif kernel == 'posterior':
        got = ('staged',) if post.host_fits(side, d, logit_bytes) else ('streamed',)
    else:
        pixels, c = side * side, d * j
        tile, chunk = marg.host_tile_pixels(pixels), marg.host_chunk_pixels(pixels, c, acc_bytes)
        assert (tile, chunk) == (G.tile_pixels(pixels), G.chunk_pixels(pixels, c, acc_bytes)), (side, j, d, precise)
        got = (f'tile{tile}', 'ragged' if pixels % tile else 'even', 'C>256' if c > 256 else 'C<=256', 'chunk<tile' if chunk < tile else 'chunk=tile')
    assert got == G.shape_class(kernel, side, j, d, precise), (kernel, side, j, d, precise, got)
    return got


def grid_heads():
    """{(head side, head joints)} of the supported grid, depth 8."""
    return sorted({(side // stride, ModelSpec(50, stride, ds, proc_side=side).skeleton.n_head)
                   for side in GRID_SIDES for stride in GRID_STRIDES for ds in GRID_DATASETS})


def required_classes(helpers):
    """{(kernel, precise, class): a head of the grid that reaches it}; the modes' refused class is no launch."""
    req = {}
    for side, j in grid_heads():
        for kernel in ('modes', 'posterior', 'marginals'):
            for precise in G.PRECISES:
                cls = kernel_class(helpers, kernel, side, j, 8, precise)
                if cls != ('refused',):
                    req.setdefault((kernel, precise, cls), (side, j))
    return req


def holders(helpers, launches):
    """{(kernel, precise, class): [case ids]} of the GPU file's launches."""
    out = {}
    for kernel, case, side, j, d, precise in launches:
        out.setdefault((kernel, precise, kernel_class(helpers, kernel, side, j, d, precise)), []).append(case)
    return out


def closure_gaps(helpers, launches):
    have = holders(helpers, launches)
    return [f'{kernel} precise {precise} {" ".join(cls)}: reached by the head of side {at[0]} with {at[1]} joints, launched by no case'
            for (kernel, precise, cls), at in sorted(required_classes(helpers).items()) if (kernel, precise, cls) not in have]


def test_the_grid_reaches_the_decisions_the_cases_are_built_around(helpers):
    heads = grid_heads()
    assert {s for s, _ in heads} >= {2, 3, 16, 44, 48, 64, 72, 80, 88, 128} and {j for _, j in heads} == {17, 19, 53}
    assert [kernel_class(helpers, 'modes', s, 17, 8, 0) for s in (40, 44, 64, 72, 80, 84, 88)] == \
        [('whole',), ('slabs', 'ragged'), ('slabs', 'ragged'), ('slabs', 'even'), ('slabs', 'ragged'), ('slabs', 'even'), ('refused',)]
    modes = helpers[0]
    assert [modes.host_slab_rows(s, 8, b) for s, b in ((64, 4), (64, 8), (80, 4), (72, 8), (84, 4))] == [13, 5, 3, 3, 1]
    assert [kernel_class(helpers, 'posterior', s, 17, 8, p) for s, p in ((45, 0), (46, 1), (31, 2), (32, 2))] == \
        [('staged',), ('streamed',), ('staged',), ('streamed',)]
    assert kernel_class(helpers, 'marginals', 45, 17, 8, 0)[0] == 'tile32' and kernel_class(helpers, 'marginals', 46, 17, 8, 0)[0] == 'tile64'
    marg = helpers[2]
    assert (marg.host_chunk_pixels(49, 424, 8), marg.host_chunk_pixels(49, 424, 4)) == (9, 19)
    # the seam rows of the GPU cases come from md_slab_rows itself
    for c in G.MODES_CASES:
        if c.claim is G.claim_seams:
            for p in c.precises:
                rows, seams = G.seam_rows(c.side, G.logit_bytes_of(p))
                assert rows == modes.host_slab_rows(c.side, c.d, G.logit_bytes_of(p)) and all(s % rows == 0 and 0 < s < c.side for s in seams)


def test_heat_volumes_closure(helpers):
    """Every class the grid reaches, per kernel and `precise`, is launched by a case of tests/test_gpu_heat_volumes.py."""
    launches = G.launches()
    req, have = required_classes(helpers), holders(helpers, launches)
    print(f'\n{len(grid_heads())} heads in the grid; {len(req)} (kernel, precise, class) required, {len(have)} launched by {len(launches)} launches')
    gaps = closure_gaps(helpers, launches)
    assert not gaps, 'classes of the grid that no GPU case launches:\n  ' + '\n  '.join(gaps)
    assert {k for k, _, _ in req} == {'modes', 'posterior', 'marginals'} and len(req) >= 3 * (3 + 2) + 16
    # the refused class is reached, and is a refusal (test_c_refusals), never a launch
    assert any(kernel_class(helpers, 'modes', s, j, 8, 0) == ('refused',) for s, j in grid_heads())
    assert not any(cls == ('refused',) for _, _, cls in have)


def test_heat_volumes_closure_notices_a_removed_case(helpers):
    """The closure is not vacuous: without the cases that hold a required class it fails, and for every class with one holder,
    without that one case."""
    launches = G.launches()
    req, have = required_classes(helpers), holders(helpers, launches)
    sole = 0
    for key in req:
        mine = set(have[key])
        kernel, precise, _ = key
        rest = [l for l in launches if not (l[0] == kernel and l[5] == precise and l[1] in mine)]
        assert any(' '.join(key[2]) in g and f'{kernel} precise {precise}' in g for g in closure_gaps(helpers, rest)), key
        sole += len(mine) == 1
    assert sole >= 3, 'no class is held by a single case: the removal of one case was not exercised'


# ---- the CPU half of the workgroup cases -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c.name for c in G.MODES_CASES])
def test_every_workgroup_case_has_the_property_it_claims(name):
    c = G.MODES_BY_NAME[name]
    for logit_bytes in sorted({G.logit_bytes_of(p) for p in c.precises}):
        lg = G.modes_case_logits(name, logit_bytes)
        assert lg.shape == (c.n, c.side, c.side, c.d * c.j) and np.array_equal(lg, G.fp32_values(lg), equal_nan=True)
        rv, rs = G.modes_case_reference(name, logit_bytes)
        c.claim(c, lg, rv, rs, logit_bytes)
        small = MR.small_fraction(rv, rs)
        print(f'{name} ({logit_bytes}-byte logits): {int((rv >= 0).sum())} modes emitted, {small:.3f} of them below {MR.SMALL_MASS:g}')
        assert small < 0.05, (name, small)


def test_the_bad_voxels_are_owned_as_stated():
    vol = G.BAD_SIDE * G.BAD_SIDE * G.BAD_D
    assert G.BAD_VOXELS[0] == 0 and G.BAD_VOXELS[1] == vol - 1 and G.owner(G.BAD_VOXELS[2]) == (255, 3, 63) and G.BAD_VOXELS[2] < vol


def test_the_host_cases_stay_within_the_cap_on_negligible_modes():
    """Per case (the GPU tests assert it case by case); the cases up to S = 20 emit no such mode at all."""
    for side, j, d, n, k, radius, _ in TM.HOST_CASES:
        small = MR.small_fraction(*TM.case_reference(side, j, d, n, k, radius, False))
        assert small < 0.05 and (side > 20 or small == 0), (side, j, d, n, k, radius, small)


@pytest.mark.parametrize('name', [c.name for c in G.POSTERIOR_CASES])
def test_every_posterior_case_has_the_property_it_claims(name):
    c = G.POSTERIOR_BY_NAME[name]
    lg, prior, ref = G.posterior_case(name)
    assert lg.shape == (c.n, c.side, c.side, c.d * c.j) and prior.shape == (c.n, c.j + 1, 9) and prior.dtype == np.float32
    c.claim(c, lg, prior, ref)
