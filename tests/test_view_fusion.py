"""The view fusion without a GPU: the fp64 restatement (tests/view_fusion_ref.py) on the two-peaked scene of the design note,
view_fusion.hip's body compiled for the host and walked by a team of one thread against the restatement (every pass of
fusion_walk; the workgroup's ladders are the one part only the GPU tests run), the C symbol and its refusals, the dispatch of
bound forwards by dry run, and the argument checks of the Python surface that run before any launch.

Bounds (view_fusion_ref): integers exact, points within 1e-3 mm, each covariance block within 1e-6 of its largest entry, peak
and agreement within 4 fp32 ulps or 1e-6; every compared case first asserts the margins that keep its decisions from
flipping.  Worst deviations measured on the host-compiled code: points 3.0e-5 mm, blocks 5.4e-8, peak 2.8e-8, agreement 4.5e-7
(the fp32 rounding of an agreement near -5)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib, heads as MH
from tests import view_fusion_ref as VF
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_MM = 1200.0 / 15                      # one step of the default grid


# ---- 1, 2: the scene of the design note, on the restatement ----------------------------------------------------------------------

def _errors(**kw):
    case, uniform, weighted = VF.scene(**kw)
    ref = VF.fuse(case)
    err = lambda x: float(np.linalg.norm(np.asarray(x, np.float64) - VF.SCENE_TRUTH))
    return dict(uniform=err(uniform), weighted=err(weighted), fused=err(ref['points'][0, 0]), agreement=float(ref['agreement'][0, 0]),
                peak=float(ref['peak'][0, 0]), edge=int(ref['edge'][0, 0]), n_rows=int(ref['n_rows'][0, 0]))


def test_two_peaked_scene():
    """Camera 0 of three carries 0.55 of its mass in a second blob 5 cells to the right: the means' triangulation is bent by it
    (uniform 240 mm, covariance-weighted 94 mm), the fused mean is not (5.8 mm).  Measured here, recorded in
    profiles/view_fusion_parity.json by tools/view_fusion_parity.py."""
    e = _errors()
    print('two-peaked scene:', e)
    assert e['n_rows'] == 3 and e['edge'] == 0
    assert e['weighted'] > 50.0, 'the scene bends the triangulation'
    assert e['fused'] <= e['weighted'] / 3.0, e
    assert e['fused'] <= STEP_MM, e


@pytest.mark.parametrize('kw', (dict(wrong_weight=0.7), dict(angles_deg=(0.0, 90.0, 180.0, 270.0))), ids=('weight-0.7', 'four-cameras'))
def test_two_peaked_scene_variants(kw):
    e = _errors(**kw)
    print('two-peaked scene', kw, e)
    assert e['fused'] <= e['weighted'] / 3.0 and e['fused'] <= STEP_MM, e


def test_clean_scene():
    """No second blob: the triangulation is exact (the rays of the means meet), the fused mean is within 10 mm, an eighth of
    the 80 mm step -- the bilinear probabilities are a coarser model than the soft-argmax, which is why the fusion is returned
    beside the triangulation."""
    e = _errors(wrong_weight=0.0)
    print('clean scene:', e)
    assert e['weighted'] < 0.5 and e['fused'] <= 10.0, e


def test_agreement():
    clean, two = _errors(wrong_weight=0.0), _errors()
    assert clean['agreement'] <= 0 and two['agreement'] <= 0
    assert clean['agreement'] > two['agreement'], (clean, two)
    for seed in range(3):
        ref = VF.fuse(VF.make_case(VF.head_of(128, 16), 3, (3, 2, 0), seed=seed, grid=8))
        used = ref['n_rows'] > 0
        assert (ref['agreement'][used] <= 0).all() and np.isnan(ref['agreement'][~used]).all()


def test_two_cameras():
    """With two cameras the wrong peak's ray still meets the other camera's ray and nothing resolves it.  That is inherent: NO
    improvement over the triangulation is asserted, only that the call is defined (a finite point inside the cube)."""
    e = _errors(angles_deg=(0.0, 120.0))
    print('two cameras:', e)
    assert e['n_rows'] == 2 and np.isfinite(e['fused'])


# ---- 3, 4: the kernel's code on the host against the restatement ------------------------------------------------------------------

@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """csrc/view_fusion.hip's fusion_walk on the host: a team of one thread, one walk per (person, output joint)."""
    lib = compile_for_host(tmp_path_factory.mktemp('view_fusion_host'), 'host_view_fusion', ['view_fusion.hip'], '''
#include <vector>
struct HostTeam {
    int tid = 0;
    static constexpr int nt = 1;
    void sync() const {}
    template <int N, typename T> void maxes(T (&)[N]) const {}
    template <int N, typename T> void sums(T (&)[N]) const {}
    void argmax(double&, int&) const {}
};
extern "C" void host_view_fusion(const float* xy, const MetroPlacement* rec, const int* rows, int n_rows, const int* starts, int n_persons,
                                 const int* mirror, const float* centres, const MetroViewFusion* params, int n, const MetroSpec* spec,
                                 float* points, float* cov, float* stats, int* info, float* centres_out) {
    using namespace metro;
    const ViewFusionArgs a = make_view_fusion_args(xy, rec, rows, n_rows, starts, n_persons, mirror, centres, *params, n, *spec, points,
                                                   cov, stats, info, centres_out);
    std::vector<double> lds(VF_LDS_BYTES / 8);
    HostTeam team;
    for (int item = 0; item < n_persons * a.n_out; ++item) fusion_walk(a, item, reinterpret_cast<char*>(lds.data()), team);
}
''')
    lib.host_view_fusion.restype = None
    lib.host_view_fusion.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.POINTER(_lib.MetroViewFusion), C.c_int, C.POINTER(_lib.MetroSpec)] + [C.c_void_p] * 5
    return lib


def fusion_record(case, weights='uniform'):
    par = case['params']
    return MH.fusion_params(par['grid'], par['extent_mm'], par['floor'], par['near_mm']).record(weights, 2.0, par['n_views'])


def run_host(host, case, cs):
    """The host-compiled kernel code on a restatement case -> (points, cov, stats, info, centres_out), pre-filled with a sentinel."""
    n_persons, n_out = len(case['starts']) - 1, len(case['mirror'])
    keep = [np.ascontiguousarray(case['xy'], np.float32), np.ascontiguousarray(case['records']), np.ascontiguousarray(case['rows'], np.int32),
            np.ascontiguousarray(case['starts'], np.int32), np.ascontiguousarray(case['mirror'], np.int32),
            np.ascontiguousarray(case['centres'], np.float32)]
    outs = [np.full((n_persons, n_out, k), -7, t) for k, t in ((3, np.float32), (9, np.float32), (2, np.float32), (2, np.int32), (3, np.float32))]
    ptr = lambda a: a.ctypes.data
    params = fusion_record(case)
    host.host_view_fusion(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), len(keep[2]), ptr(keep[3]), n_persons, ptr(keep[4]), ptr(keep[5]),
                          C.byref(params), int(case['n']), C.byref(cs), *(ptr(a) for a in outs))
    assert outs[4].tobytes() == keep[5].tobytes(), 'the centres are copied bit for bit'
    return outs


def hold(host, case, cs):
    ref = VF.fuse(case)
    worst = VF.check(run_host(host, case, cs)[:4], ref)
    print(worst, ref['margins'])
    return ref


@pytest.mark.parametrize('side', (2, 3, 16, 64))
def test_host_code_over_heat_map_sides(host, side):
    cs, head = VF.cspec(side, 3)
    ref = hold(host, VF.make_case(head, 3, (3, 4), seed=side), cs)
    assert (ref['n_rows'] == np.array([[3], [4]])).all()


@pytest.mark.parametrize('grid', (2, 3, 16))
def test_host_code_over_grids(host, grid):
    cs, head = VF.cspec(16, 3)
    ref = hold(host, VF.make_case(head, 3, (3, 4), seed=20 + grid, grid=grid), cs)
    if grid == 2:
        assert (ref['edge'] == 1).all(), 'every point of a 2 x 2 x 2 cube lies on its surface'


def test_host_code_over_rows_per_person(host):
    """0, 1, 2, 16, 17 and 33 rows: no chunk, one partly filled, one full, one full and one row, two full and one row."""
    cs, head = VF.cspec(16, 2)
    counts = (0, 1, 2, 16, 17, 33)
    ref = hold(host, VF.make_case(head, 2, counts, seed=31, grid=8), cs)
    assert (ref['n_rows'] == np.array(counts)[:, None]).all()


@pytest.mark.parametrize('n_out', (1, 17, 19))
def test_host_code_over_output_joints(host, n_out):
    cs, head = VF.cspec(16, n_out)
    hold(host, VF.make_case(head, n_out, (3, 2), seed=40 + n_out, grid=6), cs)


@pytest.mark.parametrize('n_views', (1, 3))
def test_host_code_over_views(host, n_views):
    """Three rows per camera (test-time views) each count a third: the energies of V = 3 are a third of V = 1's."""
    cs, head = VF.cspec(16, 3)
    case = VF.make_case(head, 3, (6,), seed=51, n_views=n_views, grid=8)
    ref = hold(host, case, cs)
    one = VF.fuse(dict(case, params=dict(case['params'], n_views=1)))
    np.testing.assert_allclose(ref['agreement'] * n_views, one['agreement'], rtol=1e-12)


SINGLE = ('flipped-view', 'nan-map', 'non-finite-record', 'row-index-outside', 'behind-a-camera', 'outside-the-map', 'nan-centre')


@pytest.mark.parametrize('name', SINGLE)
def test_host_code_on_single_cases(host, name):
    cs, head = VF.cspec(16, 3)
    case = VF.single_cases(head, 3)[name]
    case['behind'], case['outside'] = VF.count_floor_points(case)
    VF.check_single(name, case, hold(host, case, cs))


def test_flipped_view_needs_the_mirror_table(host):
    """The flipped-view case read without the swap (an identity mirror table) gives other numbers: the case can tell."""
    cs, head = VF.cspec(16, 3)
    case = VF.single_cases(head, 3)['flipped-view']
    with_swap, without = VF.fuse(case), VF.fuse(dict(case, mirror=np.arange(3, dtype=np.int32)))
    assert np.abs(with_swap['points'][0, :2] - without['points'][0, :2]).max() > 1.0
    assert np.abs(with_swap['points'] - case['truth']).max() < STEP_MM


def test_margin_check_refuses_a_case_on_a_border():
    """The margins hold on the scene, and a case whose nearest projection lies 1e-7 cells from a map border is refused."""
    case, _, _ = VF.scene(wrong_weight=0.0)
    ref = VF.fuse(case)
    VF.assert_margins(ref)
    ref['margins']['border'] = 1e-7
    with pytest.raises(AssertionError):
        VF.assert_margins(ref)


# ---- the Python surface, before any launch ---------------------------------------------------------------------------------------

def test_fusion_params_validates_the_keywords():
    f = MH.fusion_params()
    assert f == MH.Fusion(16, 1200.0, 1e-6, 100.0) and 'design choices, not measurements' in MH.fusion_params.__doc__
    for kw in (dict(grid=1), dict(grid=17), dict(grid=8.0), dict(grid=True), dict(extent_mm=0), dict(extent_mm=float('nan')),
               dict(floor=0.0), dict(floor=1.0), dict(floor=-1e-3), dict(near_mm=-1.0), dict(near_mm=float('inf'))):
        with pytest.raises(ValueError):
            MH.fusion_params(**kw)
    rec = MH.fusion_params(8, 900.0, 1e-4, 0.0).record('uniform', 2.0, 3)
    assert (rec.grid, rec.n_views, rec.weights, rec.extent_mm, rec.floor, rec.near_mm) == (8, 3, _lib.METRO_TRI_UNIFORM, 900.0, 1e-4, 0.0)
    assert rec.min_det == MH.triangulation_min_det('uniform', 2.0)
    for bad in (dict(weights='best'), dict(min_angle_deg=0.0), dict(n_views=0), dict(n_views=1.5)):
        with pytest.raises(ValueError):
            f.record(**dict(dict(weights='covariance', min_angle_deg=2.0, n_views=1), **bad))


def test_exports():
    import metro_pose3d_amd as M
    from metro_pose3d_amd import frames as FR
    from metro_pose3d_amd.engine import Engine
    assert M.fuse_poses_in_frames is FR.fuse_poses_in_frames and M.FusedPoses is FR.FusedPoses
    assert 'fuse_poses_in_frames' in M.__all__ and 'FusedPoses' in M.__all__
    assert FR.FusedPoses._fields == ('world', 'poses', 'covariance', 'peak', 'agreement', 'n_rows', 'edge')
    assert callable(Engine.forward_view_fusion)


def test_the_frames_call_checks_before_any_launch():
    from metro_pose3d_amd import frames as FR
    frame = [np.zeros((64, 64, 3), np.uint8)] * 2
    boxes, cams = np.array([[8.0, 8, 32, 32]] * 2), None
    with pytest.raises(ValueError, match='grid'):
        FR.fuse_poses_in_frames(frame, boxes, 'no-such-model', cams, [0, 0], [0, 1], grid=1)
    with pytest.raises(ValueError, match='floor'):
        FR.fuse_poses_in_frames(frame, boxes, 'no-such-model', cams, [0, 0], [0, 1], floor=2.0)
    with pytest.raises(ValueError, match='weights'):
        FR.fuse_poses_in_frames(frame, boxes, 'no-such-model', cams, [0, 0], [0, 1], weights='best')
    with pytest.raises(ValueError, match='calibrated cameras'):
        FR.fuse_poses_in_frames(frame, boxes, 'no-such-model', cams, [0, 0], [0, 1])


# ---- 5: the C surface --------------------------------------------------------------------------------------------------------------

def test_symbol_in_header_bindings_and_library():
    header = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    proto = re.search(r'int\s+metro_plan_bind_view_fusion\(([^;]*)\);', header).group(1)
    assert 'stream' not in proto, 'a bind entry takes no stream: no new launching entry'
    assert len(proto.split(',')) == len(_lib.SIGNATURES['metro_plan_bind_view_fusion'][1]) == 16
    assert re.search(r'#define METRO_ABI_VERSION 8\b', header) and _lib.load().metro_abi_version() == 8
    assert C.sizeof(_lib.MetroViewFusion) == 48 and _lib.MetroViewFusion.extent_mm.offset == 16
    for word in ('With TWO\n * cameras the wrong peak', 'replaces nothing'):
        assert word in header, word
    assert 'view_fusion.hip' in open(os.path.join(ROOT, 'metro_pose3d_amd', 'build.py')).read()
    assert 'metro_plan_bind_view_fusion' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def _plan(lib, spec, precision=1, max_batch=4):
    plan = C.c_void_p()
    cs = spec.to_c(precision)
    _lib.check(lib.metro_plan_create(C.byref(cs), max_batch, C.byref(plan)), 'metro_plan_create')
    return plan


NAMES = ('xy', 'records', 'rows', 'starts', 'mirror', 'centres', 'points', 'cov', 'stats', 'info', 'centres_out')


def _binder(lib, plan):
    ptrs = {name: C.c_void_p(4096 * (i + 1)) for i, name in enumerate(NAMES)}     # nothing is dereferenced at bind time
    good = MH.fusion_params().record('covariance', 2.0)

    def bind(params=good, n_rows=6, n_persons=2, max_n=4, **swap):
        p = dict(ptrs, **swap)
        return lib.metro_plan_bind_view_fusion(plan, p['xy'], p['records'], p['rows'], n_rows, p['starts'], n_persons, p['mirror'],
                                               p['centres'], C.byref(params) if params is not None else None, p['points'], p['cov'],
                                               p['stats'], p['info'], p['centres_out'], max_n)
    return bind


def _unbind(lib, plan):
    return lib.metro_plan_bind_view_fusion(plan, None, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 0)


def test_bind_refusals_one_by_one():
    """Every refusal of the bind entry returns METRO_ERR_INVALID_ARG and leaves the earlier binding in place."""
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8))
    bind = _binder(lib, plan)
    try:
        assert bind() == 0 and bind(centres=None) == 0, 'with centres, and without'
        for name in NAMES:
            if name != 'centres':
                assert bind(**{name: None}) == -1 and b'go together' in lib.metro_last_error(), name
        assert bind(params=None) == -1
        for name in NAMES:
            assert bind(**{name: C.c_void_p(4096 * 20 + 2)}) == -1 and b'aligned' in lib.metro_last_error(), name
        for max_n in (0, 5, -1):
            assert bind(max_n=max_n) == -1 and b'max_n' in lib.metro_last_error()
        assert bind(n_persons=-1) == -1 and bind(n_rows=-1) == -1
        assert bind(n_persons=0, n_rows=0) == 0, 'no persons: a binding that launches nothing'
        for field, value in (('grid', 1), ('grid', 17), ('n_views', 0), ('weights', 2), ('weights', -1), ('extent_mm', 0.0),
                             ('extent_mm', float('inf')), ('floor', 0.0), ('floor', 1.0), ('floor', float('nan')), ('near_mm', -1.0),
                             ('near_mm', float('nan')), ('min_det', float('nan'))):
            p = MH.fusion_params().record('covariance', 2.0)
            setattr(p, field, value)
            assert bind(params=p) == -1, (field, value)
            assert field.encode() in lib.metro_last_error(), (field, lib.metro_last_error())
        assert _unbind(lib, plan) == 0 and _unbind(lib, plan) == 0
        # all pointers NULL but a size left: not the unbind call
        assert lib.metro_plan_bind_view_fusion(plan, None, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 1) == -1
    finally:
        lib.metro_plan_destroy(plan)


def test_heat_map_side_below_two_has_no_plan_to_bind_to():
    """The bind entry also refuses S < 2 (a bilinear value needs four cells), but no plan reaches it: metro_plan_create refuses
    such a head first, which is what can be shown here."""
    with pytest.raises(ValueError, match='heat-map side 1'):
        _plan(_lib.load(), ModelSpec(50, 32, 'h36m', base_width=8, proc_side=32))


def test_forward_refusals_before_any_launch():
    """n > max_n; without centres a forward entry with no coords01 output, or under METRO_TRI_COVARIANCE with no cov01 output:
    METRO_ERR_INVALID_ARG from the checks that run before the first launch (the parameters are a fake blob; nothing is enqueued)."""
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8), max_batch=4)
    bind = _binder(lib, plan)
    fake = C.c_void_p(1 << 20)
    try:
        assert lib.metro_plan_bind_params(plan, fake) == 0
        assert bind(max_n=2) == 0
        assert lib.metro_forward_coords01(plan, fake, 3, fake, fake, fake, None) == -1 and b'metro_plan_bind_view_fusion' in lib.metro_last_error()
        assert bind(max_n=2, centres=None) == 0
        assert lib.metro_forward(plan, fake, 2, fake, fake, None) == -1 and b'coords01' in lib.metro_last_error()
        assert lib.metro_forward_coords01(plan, fake, 2, fake, fake, fake, None) == -1 and b'cov01' in lib.metro_last_error()
        assert lib.metro_forward_moments(plan, fake, 0, 2, fake, None, fake, fake, fake, fake, None) == -1 and b'coords01' in lib.metro_last_error()
    finally:
        lib.metro_plan_destroy(plan)


def _dry_ids(lib, plan, n):
    """What metro_forward_moments with every output enqueues, by dry run (nothing is launched, no pointer is read)."""
    dry = C.c_void_p(4096)
    _lib.check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        _lib.check(lib.metro_forward_moments(plan, dry, 0, int(n), dry, dry, dry, dry, dry, dry, None), 'metro_forward_moments (dry run)')
        return lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)


@pytest.mark.parametrize('precision', ('f16', 'f32'))
def test_dispatch_of_bound_forwards_by_dry_run(precision):
    """Bound without centres, the triangulation and view_fusion<g..> end the forward's launch list, behind the marginal launches
    when those are bound; with centres, view_fusion alone; with no persons, nothing; unbound, the plan's own list again."""
    from metro_pose3d_amd.engine import Engine
    from tests.test_gpu_heat_marginals import HEAT_IDS
    lib = _lib.load()
    eng = Engine(ModelSpec(50, 16, 'h36m'), None, precision, max_batch=64)
    plan, dry = eng._plan, C.c_void_p(4096)
    bind = _binder(lib, plan)
    _lib.check(lib.metro_plan_bind_params(plan, dry), 'metro_plan_bind_params')
    try:
        for n in (1, 3, 16, 64):
            plain = _dry_ids(lib, plan, n)
            assert 'view_fusion' not in plain and 'triangulate' not in plain
            assert bind(max_n=64, centres=None) == 0
            assert _dry_ids(lib, plan, n) == plain + ' & triangulate_joints & view_fusion<g16>', n
            assert bind(max_n=64) == 0
            assert _dry_ids(lib, plan, n) == plain + ' & view_fusion<g16>', n
            _lib.check(lib.metro_plan_bind_heatmaps(plan, dry, dry, dry, 64), 'bind')
            assert _dry_ids(lib, plan, n) == ' & '.join((plain, HEAT_IDS[precision], 'view_fusion<g16>')), n
            _lib.check(lib.metro_plan_bind_heatmaps(plan, None, None, None, 0), 'unbind')
            assert bind(max_n=64, n_persons=0, n_rows=0) == 0 and _dry_ids(lib, plan, n) == plain, 'no persons, no launch'
            assert _unbind(lib, plan) == 0
            assert _dry_ids(lib, plan, n) == plain, 'unbind restores the launch list'
    finally:
        lib.metro_plan_bind_heatmaps(plan, None, None, None, 0)
        _unbind(lib, plan)
        eng.close()
