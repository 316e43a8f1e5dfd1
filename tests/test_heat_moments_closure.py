"""The MOMENTS instantiations of the head and soft-argmax launches (what return_uncertainty=True runs) against the plan's
dispatch, without a GPU.

metro_forward_moments launches, per head, the kernel the plain forward would with MOMENTS compiled in: separately compiled
kernels with a joint blocking of their own.  Which one depends on the head's side, its joint count and the call size, as for
the plain ids (tests/test_kernel_coverage.py).  This file scans the supported grid of test_dispatch_closure with dry runs of
the two kernel-level entry points (metro_kernel_notes(2): nothing is launched) -- metro_head_f16_moments for heads of whole
64-pixel tiles, metro_softargmax01_moments for the others -- and

  * ties every moments id to the plan's plain id of the same (spec, call size);
  * derives from the scan the GPU cases of tests/test_gpu_heat_moments_closure.py (HEAD_CLOSURE_CASES, SA_CLOSURE_CASES): the
    smallest call that reaches each point the closure below requires, so a new head variant cannot enter without a case;
  * requires the GPU cases to launch what the closure states (test_moments_closure).
"""
import ctypes as C

import pytest

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests.test_kernel_coverage import GRID_ARCHS, GRID_BATCHES, GRID_DATASETS, GRID_SIDES, GRID_STRIDES, DryRun, spec_name

_DRY = C.c_void_p(4096)         # any non-NULL pointer: a dry run launches nothing
SA_N = 3                        # crops of a two-launch soft-argmax case
# the two-launch soft-argmax with moments: one side per branch of softargmax_partial / softargmax_finalize, every head
#   2   4 pixels: fewer than the 6 or 7 pixel lanes of a block (2 lanes with 53 joints), the empty lanes merged by the parallel-axis update
#   4   16 pixels, one slab; with 53 joints C = 424 > 256: the channel fold loops twice
#   7   one ragged slab (49 pixels)            18   10 slabs that do not divide 324 pixels
#   36  40 slabs, a ragged last one, the 1024-thread finalize
SA_SIDES = {2: (64, 32), 4: (128, 32), 7: (224, 32), 18: (288, 16), 36: (288, 8)}          # side: (proc_side, stride) of the grid
SA_FIXED = [(side, ds) for side in SA_SIDES for ds in GRID_DATASETS]

# What the scan is expected to find (test_moments_closure): the moments head ids of the grid with their joint counts, and per
# tile width the smallest call that brings an id to each required head side -- 8 .. 64 are proc_side 256; 24 / 48 the smallest
# side that is not a power of two, 128 the largest (a 128- or 256-pixel-tile launch needs 256 tiles: n * side^2 / tile >= 256)
HEAD_JOINTS = {'head_f16<144x64,k4,moments>': 17, 'head_f16<160x64,k4,moments>': 19, 'head_f16<160x64,k4,g3,moments>': 53,
               'head_f16<144x128,k4,moments>': 17, 'head_f16<160x128,k4,moments>': 19, 'head_f16<160x128,k4,g3,moments>': 53,
               'head_f16<144x256,k2,moments>': 17, 'head_f16<160x256,moments>': 19}
SMALLEST_CALL = {'64': {8: 1, 16: 1, 24: 1, 32: 1, 64: 1, 128: 1},
                 '128': {16: 128, 32: 32, 48: 15, 64: 8, 128: 2},
                 '256': {16: 256, 32: 64, 48: 29, 64: 16, 128: 4}}
TWO_LAUNCH = 'softargmax_partial<acc32,logits32,moments> & softargmax_finalize<acc32,moments>'


def with_moments(kid):
    """A plain id (or 'a & b') with ',moments' in front of every closing bracket."""
    return ' & '.join(k[:k.rindex('>')] + ',moments' + k[k.rindex('>'):] for k in kid.split(' & '))


def whole_tiles(spec):
    return (spec.heatmap_side * spec.heatmap_side) % 64 == 0


def dry_moments_ids(lib, spec, n, c_in=2048):
    """The ids a moments call of n crops would note: the one-launch head for heads of whole 64-pixel tiles, else the two-launch
    soft-argmax (fp32 accumulators, what the f16 path runs).  Nothing is launched."""
    cs = spec.to_c(_lib.METRO_PREC_F16)
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        if whole_tiles(spec):
            check(lib.metro_head_f16_moments(_DRY, _DRY, _DRY, _DRY, _DRY, int(n), int(c_in), C.byref(cs), _DRY, _DRY, None, None, None,
                                             _DRY, _DRY, None), 'metro_head_f16_moments (dry run)')
        else:
            check(lib.metro_softargmax01_moments(_DRY, int(n), C.byref(cs), 0, _DRY, _DRY, _DRY, _DRY, _DRY, None),
                  'metro_softargmax01_moments (dry run)')
        return lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)


def point_key(ids, spec):
    return (ids, spec.heatmap_side, spec.skeleton.n_head, spec.depth)


_SCAN = {}


def moments_scan():
    """One dry run of the whole grid per process -> dict with
    points    {(ids, head side, n_joints_head, depth): (spec, n)}: the smallest call that reaches the point (then a spec of
              proc_side 256, then the first of the scan); ResNet-50 specs (the head does not see the backbone)
    at256     the points that proc_side 256 reaches
    untied    [(spec name, n, moments ids, the plan's ids)] where the moments ids are not the plan's with ',moments' inserted"""
    if _SCAN:
        return _SCAN
    lib = _lib.load()
    points, rank, at256, untied = {}, {}, set(), []
    order = 0
    for side in GRID_SIDES:
        for stride in GRID_STRIDES:
            for ds in GRID_DATASETS:
                for arch in GRID_ARCHS:
                    spec = ModelSpec(arch, stride, ds, proc_side=side)
                    run = DryRun(spec)
                    li = run.names.index('logits')
                    assert run.names[li + 1:] == ['softargmax'], run.names[li:]
                    c_in = run.infos[li].c_in
                    order += 1
                    for n in GRID_BATCHES:
                        ids = dry_moments_ids(lib, spec, n, c_in)
                        k_logits, k_soft = run.kernels(n, (li, li + 1))
                        want = with_moments(f'{k_logits} & {k_soft}' if whole_tiles(spec) else k_soft)
                        if ids != want or whole_tiles(spec) != k_logits.startswith('head_f16<'):
                            untied.append((spec_name(spec), n, ids, f'{k_logits} & {k_soft}'))
                        if arch != GRID_ARCHS[0]:
                            continue
                        key = point_key(ids, spec)
                        if side == 256:
                            at256.add(key)
                        r = (n, side != 256, order)
                        if key not in rank or r < rank[key]:
                            rank[key], points[key] = r, (spec, n)
    _SCAN.update(points=points, at256=at256, untied=untied)
    return _SCAN


def _pow2(v):
    return v & (v - 1) == 0


def required_points(scan):
    """The closure's GPU requirement -> {key: why}: every point of proc_side 256, and for every id the point of its smallest
    head side that is not a power of two and of its largest head side (the smallest call among the joint counts there)."""
    pts = scan['points']
    req = {k: 'proc_side 256' for k in scan['at256']}
    for ids in sorted({k[0] for k in pts}):
        mine = [k for k in pts if k[0] == ids]
        odd = [k[1] for k in mine if not _pow2(k[1])]
        for side, why in ((min(odd) if odd else None, 'smallest side that is not a power of two'), (max(k[1] for k in mine), 'largest side')):
            if side is None:
                continue
            at = [k for k in mine if k[1] == side]
            if not any(k in req for k in at):
                req[min(at, key=lambda k: (pts[k][1], k))] = why
    return req


def _head_cases():
    """(spec, n, ids) of the one-launch head: every required point of a head id, at the smallest call that reaches it."""
    scan = moments_scan()
    out = []
    for key, why in sorted(required_points(scan).items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2])):
        if key[0].startswith('head_f16<'):
            spec, n = scan['points'][key]
            out.append(pytest.param(spec, n, key[0], id=f'{spec_name(spec)}-b{n}:{key[0].split(" & ")[0]}'))
    return out


def _sa_cases():
    """(spec, n) of the two-launch soft-argmax: SA_FIXED, then the required points of its id that those do not launch."""
    specs = [ModelSpec(GRID_ARCHS[0], SA_SIDES[side][1], ds, proc_side=SA_SIDES[side][0]) for side, ds in SA_FIXED]
    lib, scan = _lib.load(), moments_scan()
    have = {point_key(dry_moments_ids(lib, s, SA_N), s) for s in specs}
    for key in sorted(required_points(scan)):
        if not key[0].startswith('head_f16<') and key not in have:
            specs.append(scan['points'][key][0])
    return [pytest.param(s, SA_N, id=f'{spec_name(s)}-side{s.heatmap_side}-J{s.skeleton.n_head}') for s in specs]


try:
    HEAD_CLOSURE_CASES = _head_cases()
    SA_CLOSURE_CASES = _sa_cases()
except Exception as e:  # noqa: BLE001  (library not built: the CPU tests below report it)
    HEAD_CLOSURE_CASES = [pytest.param(None, 0, str(e), id='library-missing')]
    SA_CLOSURE_CASES = [pytest.param(None, 0, id='library-missing')]


def launched_points(lib, head_cases, sa_cases):
    """{key: case id} of what the GPU cases launch, from a dry run of each case at its own (spec, call size) -- not from the id
    a case states."""
    out = {}
    for p in head_cases:
        spec, n, _ = p.values
        out.setdefault(point_key(dry_moments_ids(lib, spec, n), spec), p.id)
    for p in sa_cases:
        spec, n = p.values
        out.setdefault(point_key(dry_moments_ids(lib, spec, n), spec), p.id)
    return out


def closure_gaps(lib, scan, head_cases, sa_cases):
    """What test_moments_closure asserts, as lists of messages (empty = closed)."""
    pts = scan['points']
    launched = launched_points(lib, head_cases, sa_cases)
    at = lambda k: f'{k[0]} at head side {k[1]}, {k[2]} joints, depth {k[3]}: {spec_name(pts[k][0])}, batch {pts[k][1]}'
    ids = {k[0] for k in launched}
    no_id = sorted({k[0]: at(k) for k in sorted(pts, key=lambda k: -pts[k][1]) if k[0] not in ids}.values())
    no_point = [f'{at(k)} ({why})' for k, why in sorted(required_points(scan).items()) if k not in launched]
    return no_id, no_point


def test_moments_ids_are_the_plans_ids_with_moments_compiled_in():
    """At every point of the grid of test_dispatch_closure (proc_side 64 .. 512 x ResNet-v2 50 / 101 x stride 4 .. 32 x three heads x
    every call size 1 .. 256) the ids the moments entry points note are the plan's plain `logits` / `softargmax` ids with
    ',moments' in front of the closing bracket -- of both names on the two-launch path -- and a head takes the one-launch path
    exactly when it is whole 64-pixel tiles.  What metro_forward_moments dispatches is thereby what the plan names."""
    scan = moments_scan()
    assert not scan['untied'], f'{len(scan["untied"])} grid points; the first:\n' + \
        '\n'.join(f'  {s}, batch {n}: moments ids {ids!r}, the plan names {plan!r}' for s, n, ids, plan in scan['untied'][:10])
    assert with_moments('head_f16<160x128,k4,g3> & softargmax_finalize<acc32>') == 'head_f16<160x128,k4,g3,moments> & softargmax_finalize<acc32,moments>'
    assert all(',moments>' in part for k in scan['points'] for part in k[0].split(' & '))


def test_the_notes_string_holds_a_whole_forward(lib):
    """metro_kernel_notes(1) around metro_forward_moments is how the GPU tests read which head a forward dispatched: the string
    must hold every launch of the longest plan of the grid, and one that does not fit must say so."""
    longest = max(len(' & '.join(DryRun(ModelSpec(arch, stride, 'merged'), 16).kernels(16))) for arch in GRID_ARCHS for stride in GRID_STRIDES)
    spec = ModelSpec(50, 32, 'h36m', proc_side=224)
    cs = spec.to_c(_lib.METRO_PREC_F16)
    one = with_moments('softargmax_partial<acc32,logits32> & softargmax_finalize<acc32>')
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        calls = 0
        while (calls + 1) * (len(one) + 3) <= longest + 2 * len(',moments') + len(one):
            check(lib.metro_softargmax01_moments(_DRY, 2, C.byref(cs), 0, _DRY, _DRY, _DRY, _DRY, _DRY, None), 'dry run')
            calls += 1
        assert lib.metro_last_kernel_id().decode() == ' & '.join([one] * calls), 'a string as long as the longest forward\'s was cut'
        for _ in range(4096 // len(one)):
            check(lib.metro_softargmax01_moments(_DRY, 2, C.byref(cs), 0, _DRY, _DRY, _DRY, _DRY, _DRY, None), 'dry run')
        assert lib.metro_last_kernel_id().decode().endswith('> ...')
    finally:
        lib.metro_kernel_notes(0)


def test_moments_closure(lib):
    """Every MOMENTS instantiation the supported grid reaches is launched by a GPU case of tests/test_gpu_heat_moments_closure.py
    (HEAD_CLOSURE_CASES: one metro_head_f16_moments launch each; SA_CLOSURE_CASES: the two-launch soft-argmax), and

      * every (ids, head side, n_joints_head, depth) point that proc_side 256 reaches is launched (the level of test_pair_closure);
      * for every id, so are its point with the smallest head side that is not a power of two (32-pixel slabs cross image
        rows there, and the moments need every pixel's (x, y)) and its point with the largest head side.

    The stated limit: the other sides of the grid stay at the level of ids -- the whole grid has some hundred points, which
    differ in the map side only.  What a case launches is taken from a dry run at its own call size."""
    assert HEAD_CLOSURE_CASES[0].values[0] is not None, f'libmetro_hip.so could not be loaded at collection time: {HEAD_CLOSURE_CASES[0].values[2]}'
    scan = moments_scan()
    no_id, no_point = closure_gaps(lib, scan, HEAD_CLOSURE_CASES, SA_CLOSURE_CASES)
    req = required_points(scan)
    print(f'\n{len({k[0] for k in scan["points"]})} moments ids, {len(scan["points"])} (ids, side, joints, depth) points in the grid, '
          f'{len(scan["at256"])} of them at proc_side 256; {len(req)} required, {len(HEAD_CLOSURE_CASES)} head cases + '
          f'{len(SA_CLOSURE_CASES)} soft-argmax cases')
    assert not no_id, 'moments ids of the grid that no GPU case launches (largest call that reaches each):\n  ' + '\n  '.join(no_id)
    assert not no_point, 'required points that no GPU case launches (smallest call that reaches each):\n  ' + '\n  '.join(no_point)
    # every case states the ids its own dry run names
    for p in HEAD_CLOSURE_CASES:
        assert dry_moments_ids(lib, p.values[0], p.values[1]) == p.values[2], p.id
    # the derived list follows the dispatch by itself; what it is derived FROM is pinned, so a new branch of head_f16_variant (a new
    # id, or an id at another call size) is a decision someone states here, with the GPU cases it brings reviewed and run
    got = {}
    for (ids, side, nj, _), _ in req.items():
        if ids.startswith('head_f16<'):
            head = ids.split(' & ')[0]
            assert ids == f'{head} & softargmax_finalize<acc32,moments>' and HEAD_JOINTS[head] == nj, (ids, nj)
            got.setdefault(head, {})[side] = scan['points'][(ids, side, nj, 8)][1]
    want = {head: SMALLEST_CALL[head.split('x')[1].split(',')[0]] for head in HEAD_JOINTS}
    assert got == want, 'the dispatch of the moments heads moved: {head id: {head side: smallest call}}\n' + \
        '\n'.join(f'  {h}: now {got.get(h)}, stated {want.get(h)}' for h in sorted(set(got) | set(want)) if got.get(h) != want.get(h))
    assert {k[0] for k in scan['points']} == {f'{h} & softargmax_finalize<acc32,moments>' for h in HEAD_JOINTS} | {TWO_LAUNCH}


def test_moments_closure_notices_a_deleted_case_and_a_new_variant(lib):
    """The closure is not vacuous: without any one head case a required point is unlaunched, and an id the scan would name for
    a new branch of the dispatch (here: a made-up tile width at one grid point) is reported as launched by no case."""
    scan = moments_scan()
    for i in range(len(HEAD_CLOSURE_CASES)):
        no_id, no_point = closure_gaps(lib, scan, HEAD_CLOSURE_CASES[:i] + HEAD_CLOSURE_CASES[i + 1:], SA_CLOSURE_CASES)
        assert no_point, f'the closure holds without {HEAD_CLOSURE_CASES[i].id}'
    key = next(k for k in sorted(scan['points']) if k[0].startswith('head_f16<'))
    grown = dict(scan, points=dict(scan['points']))
    grown['points'][('head_f16<160x512,k1,moments> & softargmax_finalize<acc32,moments>',) + key[1:]] = scan['points'][key]
    no_id, _ = closure_gaps(lib, grown, HEAD_CLOSURE_CASES, SA_CLOSURE_CASES)
    assert len(no_id) == 1 and 'head_f16<160x512,k1,moments>' in no_id[0], no_id
