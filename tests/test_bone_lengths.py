"""metro_track_bone_lengths without a GPU: the fp64 restatement (tests/bone_lengths_ref.py) on known answers, bone_lengths.hip's
own __host__ __device__ functions compiled for the host and held to the restatement, and the argument checks of the C entry, of
heads.track_bone_lengths, of frames.Follower(learn_bones=...) and of locate_poses_in_frames' device bone lengths -- all before
the library launches anything."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from metro_pose3d_amd.joints import skeleton
from tests import bone_lengths_ref as BL
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on known answers ---------------------------------------------------------------------------------------------

def _one_track(poses, cov, edges, mirror, **params):
    """The restatement on float64 arrays as they are, one track that owns every row -> (table, lengths, sigma, known)."""
    p = dict(BL.DEFAULTS, **params)
    table = BL.new_table(1, len(edges))
    BL.update(table, poses, cov, np.arange(len(poses)), [0, len(poses)], [0], edges, **p)
    return (table,) + BL.read_out(table, mirror, None, p['min_count'], p['symmetric'])


def test_rigid_skeleton_gives_its_lengths():
    sk, edges, mirror = BL.h36m()
    rng = np.random.default_rng(1)
    base = rng.normal(size=(sk.n_out, 3)) * 300.0
    poses = np.stack([base @ BL.rotation(rng).T + rng.normal(size=3) * 3000.0 for _ in range(20)])
    true = np.linalg.norm(base[edges[:, 1]] - base[edges[:, 0]], axis=1)
    _, lengths, sigma, known = _one_track(poses, None, edges, mirror, symmetric=False)
    assert known.all() and np.abs(lengths[0] / true - 1.0).max() <= 1e-9
    assert np.allclose(sigma[0], np.sqrt(1.0 / 20.0), rtol=1e-12)          # 20 rows at v = sigma_floor_mm^2 = 1


def test_two_rows_give_the_closed_form_weighted_mean():
    """C_a + C_b = c I: tr C / 3 = c, tr C - u^T C u = 2 c, so v = c + 1 and l^ = l - c / l."""
    edges, mirror = np.array([[0, 1]]), np.array([-1])
    poses = np.array([[[0.0, 0, 0], [300.0, 0, 0]], [[10.0, 20, 30], [10.0, 20 + 180.0, 30 + 240.0]]])      # l = 300 and 300
    poses[1, 1] += [0.0, 6.0, 8.0]                                                                          # l = 310
    cov = np.zeros((2, 2, 3, 3))
    cov[0, :] = 12.0 * np.eye(3)          # c = 24
    cov[1, :] = 49.5 * np.eye(3)          # c = 99
    a, b = 25.0, 100.0
    la, lb = 300.0 - 24.0 / 300.0, 310.0 - 99.0 / 310.0
    _, lengths, sigma, known = _one_track(poses, cov, edges, mirror, min_count=2)
    assert known[0, 0] == 1
    assert abs(lengths[0, 0] - (la / a + lb / b) / (1 / a + 1 / b)) <= 1e-12 * 300
    assert abs(sigma[0, 0] - np.sqrt(1.0 / (1 / a + 1 / b))) <= 1e-12
    _, lengths, _, _ = _one_track(poses, cov, edges, mirror, min_count=2, debias=False)
    assert abs(lengths[0, 0] - (300.0 / a + 310.0 / b) / (1 / a + 1 / b)) <= 1e-12 * 300
    assert _one_track(poses, cov, edges, mirror, min_count=3)[3][0, 0] == 0


@pytest.mark.parametrize('seed', range(5))
def test_debiased_length_of_a_noisy_bone(seed):
    """A 250 mm bone along (0.6, 0, 0.8), joint noise N(0, s^2 diag(8, 8, 30)^2) and N(0, s^2 diag(10, 10, 35)^2) mm, s ~ U(0.5, 3)
    per row, 20 000 rows, the gate off: the debiased error is at most 1 mm and at most a third of the naive one.
    Measured on the restatement with np.random.default_rng(seed), debiased / naive error in mm:
    seed 0 -0.319 / +3.464, seed 1 -0.397 / +3.309, seed 2 +0.151 / +3.859, seed 3 -0.395 / +3.317, seed 4 -0.227 / +3.503
    (about a dozen of the 20 000 rows are skipped for l^ <= 0, as the model says)."""
    poses, cov = BL.bias_scene(seed)
    edges, mirror = np.array([[0, 1]]), np.array([-1])
    debiased = _one_track(poses, cov, edges, mirror, gate=0.0)[1][0, 0] - 250.0
    naive = _one_track(poses, cov, edges, mirror, gate=0.0, debias=False)[1][0, 0] - 250.0
    print(f'seed {seed}: debiased {debiased:+.3f} mm, naive {naive:+.3f} mm')
    assert abs(debiased) <= 1.0 and abs(debiased) <= abs(naive) / 3.0


def test_an_outlier_is_gated_after_min_count_and_accepted_before():
    for position, rejected in ((10, 1), (3, 0)):
        case, edge = BL.outlier_case(position)
        table, after, (lengths, _, known) = BL.run(case)
        assert after[-1][0, edge, 3] == rejected and after[-1][0, edge, 2] == 11 - rejected
        assert after[-1][0, :, 3].sum() == rejected and known.all()
        if rejected:                                        # the one decision that rejects lies far from its threshold
            assert min(table['margins']) >= 1e-6 and max(table['margins']) > 1.0


def test_mirror_pooling_and_fallback():
    case, left = BL.arm_case(True)
    _, after, (lengths, sigma, known) = BL.run(case)
    dead = np.flatnonzero(np.isin(case['edges'], left).any(1))
    assert len(dead) == 2 and (after[-1][:, dead, 2] == 0).all()
    partner = case['mirror'][dead]
    assert (partner >= 0).all() and known[:, dead].all()
    assert np.array_equal(lengths[:, dead], lengths[:, partner]) and np.array_equal(sigma[:, dead], sigma[:, partner])
    case, _ = BL.arm_case(False)
    _, _, (lengths, sigma, known) = BL.run(case)
    assert (known[:, dead] == 0).all() and np.isnan(sigma[:, dead]).all()
    assert np.array_equal(lengths[:, dead], np.tile(case['fallback'][dead], (2, 1))) and known[:, partner].all()


def test_edge_mirror_of_the_skeletons():
    sk = skeleton('h36m')
    m = sk.edge_mirror()
    name = lambda e: frozenset(sk.names[j] for j in sk.edges[e])
    assert len(m) == len(sk.edges) == len(sk.head_edges)
    for e, p in enumerate(m):
        if p >= 0:
            assert m[p] == e and p != e
            assert name(p) == frozenset(('r' if n[0] == 'l' else 'l' if n[0] == 'r' else n[0]) + n[1:] for n in name(e))
    assert name(m[[set(e) for e in map(name, range(len(m)))].index({'lelb', 'lwri'})]) == {'relb', 'rwri'}
    assert m[[set(e) for e in map(name, range(len(m)))].index({'htop', 'head'})] == -1
    for dataset in ('merged', 'many19'):
        sk = skeleton(dataset)
        m = sk.edge_mirror()
        assert all(p == -1 or m[p] == e for e, p in enumerate(m)) and any(p >= 0 for p in m)


# ---- the kernel's own functions, compiled for the host --------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """bone_lengths.hip's functions are __host__ __device__: per slot, every lane's walk into the workgroup's LDS copy (on the
    stack here), the id written after all of them, then every lane's read-out -- the kernel's own order."""
    tmp = tmp_path_factory.mktemp('host_bone_lengths')
    fn = compile_for_host(tmp, 'host_bone_lengths', ['bone_lengths.hip'], '''
extern "C" void host_track_bone_lengths(const float* poses, const float* cov, int n, const int* rows, int n_rows, const int* starts,
                                        int n_tracks, const int* ids, int n_joints, const int* edges, const int* edge_mirror,
                                        int n_edges, const double* fallback, int min_count, double gate, double r_floor,
                                        double cov_scale, double min_length, int debias, int symmetric, double* stats, int* bone_ids,
                                        double* lengths, double* sigma, unsigned char* known) {
    const metro::BoneArgs a = metro::make_bone_args(poses, cov, n, rows, n_rows, starts, n_tracks, ids, n_joints, edges, edge_mirror,
                                                    n_edges, fallback, min_count, gate, r_floor, cov_scale, min_length, debias,
                                                    symmetric, stats, bone_ids, lengths, sigma, known);
    for (int t = 0; t < n_tracks; ++t) {
        metro::BoneStat slot[metro::BONE_THREADS];
        const bool fresh = bone_ids[t] != ids[t];
        for (int e = 0; e < n_edges; ++e) slot[e] = metro::bone_track_edge(a, t, e, fresh);
        if (fresh) bone_ids[t] = ids[t];
        for (int e = 0; e < n_edges; ++e) metro::bone_read_out(a, slot, t, e);
    }
}
''').host_track_bone_lengths
    fn.restype = None
    fn.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                    C.c_int, C.c_void_p, C.c_int] + [C.c_double] * 4 + [C.c_int] * 2 + [C.c_void_p] * 5)

    def run(case):
        """Every call of the case on a fresh table -> ([stats after each call], bone_ids, (lengths, sigma, known) of the last)."""
        T, E = case['T'], len(case['edges'])
        p = case['params']
        stats, bone_ids, after = np.zeros((T, E, 4)), np.full(T, -1, np.int32), []
        lengths, sigma, known = np.full((T, E), -7.0), np.full((T, E), -7.0), np.full((T, E), 7, np.uint8)
        ptr = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)
        edges, mirror = np.ascontiguousarray(case['edges'], np.int32), np.ascontiguousarray(case['mirror'], np.int32)
        for call in case['calls']:
            poses = None if call['poses'] is None else np.ascontiguousarray(call['poses'], np.float32)
            n, nj = (0, 1) if poses is None else poses.shape[:2]
            fn(ptr(poses), ptr(call['cov']), n, ptr(call['rows']), len(call['rows']) if n else 0, ptr(call['starts']), T,
               ptr(call['ids']), nj, ptr(edges), ptr(mirror), E, ptr(case['fallback']), p['min_count'], p['gate'], p['sigma_floor_mm'],
               p['cov_scale'], p['min_length_mm'], int(p['debias']), int(p['symmetric']), ptr(stats), ptr(bone_ids), ptr(lengths),
               ptr(sigma), ptr(known))
            after.append(stats.copy())
        return after, bone_ids, (lengths, sigma, known)
    return run


def _held(host_kernel, case, what):
    after, bone_ids, out = host_kernel(case)
    worst = BL.compare(after[-1], out, case, what)
    assert np.array_equal(bone_ids, case['calls'][-1]['ids'])
    print(f'{what}: worst relative deviation {worst:.2e}')
    return after, out


@pytest.mark.parametrize('name', list(BL.SHAPES))
def test_host_kernel_at_the_loop_boundaries(host_kernel, name):
    """T = 1, 2, 65, 128; E = 1, 16, 63, 64; 0, 1, 2 and 65 rows per slot; J = 1, 17, 64; with the rows the model skips: the indices
    -1 and n, a zero-length edge, NaN joints, NaN and negative-variance covariances."""
    case = BL.shape_case(name)
    call = case['calls'][0]
    assert -1 in call['rows'] and len(call['poses']) in call['rows']
    assert (case['edges'][:, 0] == case['edges'][:, 1]).any()
    if case['edges'].max() > 0:
        assert np.isnan(call['poses']).any() and np.isnan(call['cov']).any() and (call['cov'][..., 4] < 0).any()
    after, (lengths, _, known) = _held(host_kernel, case, name)
    zero = case['edges'][:, 0] == case['edges'][:, 1]
    assert (after[-1][:, zero, 2] == 0).all()
    if name != 'T1-E1-J1':
        assert known.any() and not known.all() and after[-1][..., 3].sum() > 0
        assert np.array_equal(lengths[known == 0], np.broadcast_to(case['fallback'], lengths.shape)[known == 0])


@pytest.mark.parametrize('name', ['isotropic', 'arm-pooled', 'arm-alone', 'outlier-late', 'outlier-early', 'forget', 'accumulate', 'bias'])
def test_host_kernel_matches_the_restatement(host_kernel, name):
    case = {'isotropic': BL.isotropic_case, 'arm-pooled': lambda: BL.arm_case(True)[0], 'arm-alone': lambda: BL.arm_case(False)[0],
            'outlier-late': lambda: BL.outlier_case(10)[0], 'outlier-early': lambda: BL.outlier_case(3)[0],
            'forget': lambda: BL.forget_case(True), 'accumulate': lambda: BL.forget_case(False), 'bias': lambda: BL.bias_case(0)}[name]()
    after, _ = _held(host_kernel, case, name)
    if name in ('forget', 'accumulate'):
        first, last = after[0][..., 2], after[-1][..., 2]
        assert (first[0] > 0).any() and (last[0] > first[0]).any(), 'slot 0 keeps its id and accumulates'
        if name == 'forget':
            assert (last[1] <= 14).all() and (first[1] + last[1] > 14).any(), 'slot 1 starts again under its new id'
        else:
            assert (last[1] > 14).any()


def test_a_cut_stream_leaves_the_same_stats_bit_for_bit(host_kernel):
    whole = host_kernel(BL.cut_case(None))
    assert (whole[0][-1][..., 2] > 0).any()
    for steps in BL.CUTS[1:]:
        case = BL.cut_case(steps)
        assert len(case['calls']) == -(-20 // steps)
        cut = host_kernel(case)
        assert np.array_equal(cut[0][-1].view(np.int64), whole[0][-1].view(np.int64)), steps
        for a, b in zip(cut[2], whole[2]):
            assert np.array_equal(a, b, equal_nan=True), steps
    BL.compare(whole[0][-1], whole[2], BL.cut_case(None), 'whole')


def test_read_out_alone_resets_and_reads(host_kernel):
    """No rows: the launch still resets the slots whose id changed and reads every slot out."""
    case = BL.forget_case(False)
    quiet = dict(case['calls'][1], poses=None, cov=None, rows=np.zeros(0, np.int32), ids=case['calls'][0]['ids'] + np.array([0, 9], np.int32))
    case['calls'] = [case['calls'][0], quiet]
    after, bone_ids, (lengths, sigma, known) = host_kernel(case)
    assert np.array_equal(after[1][0].view(np.int64), after[0][0].view(np.int64)) and (after[1][1] == 0).all() and (after[0][1] != 0).any()
    assert known[0].any() and not known[1].any() and np.array_equal(lengths[1], case['fallback']) and np.isnan(sigma[1]).all()
    BL.compare(after[-1], (lengths, sigma, known), case, 'read-out alone')


# ---- the surface, before the library launches anything -----------------------------------------------------------------------------------

def test_symbol_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    params = re.search(r'\bmetro_track_bone_lengths\s*\(([^)]*)\)', text).group(1)
    assert len(_lib.SIGNATURES['metro_track_bone_lengths'][1]) == params.count(',') + 1 == 26 and hasattr(lib, 'metro_track_bone_lengths')
    assert lib.metro_abi_version() == 8 and _lib.ABI_VERSION == 8            # the ABI is additive
    from metro_pose3d_amd.build import SOURCES
    assert 'bone_lengths.hip' in SOURCES


def test_c_entry_rejects_bad_arguments(lib):
    """Every -1 below comes before any launch: no device is needed; the accepted call is a dry run."""
    p = C.c_void_p(256)
    fn = lib.metro_track_bone_lengths
    good = [p, p, 8, p, 8, p, 4, p, 17, p, p, 16, None, 8, 9.0, 1.0, 1.0, 1.0, 1, 1, p, p, p, p, p, None]

    def call(**changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)
    for k, word in ((6, b'track slots'), (11, b'edges'), (8, b'n_joints_out')):
        for bad in (0, -1, 129 if k == 6 else 65):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for k in (2, 4):
        assert call(**{f'a{k}': -1}) == -1 and b'negative' in lib.metro_last_error()
    assert call(a13=0) == -1 and b'min_count' in lib.metro_last_error()
    nan, inf = float('nan'), float('inf')
    for k, word, bads in ((14, b'gate', (-1.0, nan, inf)), (15, b'r_floor', (0.0, -1.0, nan, inf)), (16, b'cov_scale', (-1.0, nan, inf)),
                          (17, b'min_length_mm', (-1.0, nan, inf))):
        for bad in bads:
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for k in (7, 9, 10, 20, 21, 22, 23, 24):                # ids, edges, edge_mirror, stats, bone_ids, the three outputs
        assert call(**{f'a{k}': None}) == -1 and b'NULL ids' in lib.metro_last_error()
    for k in (0, 3, 5):                                     # poses, rows, starts with rows to read
        assert call(**{f'a{k}': None}) == -1 and b'need poses' in lib.metro_last_error()
    lib.metro_kernel_notes(2)                               # dry run: the launcher records its id and touches no device
    try:
        assert call() == 0 and b'track_bone_lengths' in lib.metro_last_kernel_id()
        assert call(a1=None) == 0 and call(a12=p) == 0                       # isotropic; with a fallback
        assert call(a0=None, a3=None, a5=None, a2=0, a4=0) == 0              # no rows: reset and read-out only
    finally:
        lib.metro_kernel_notes(0)


def test_follower_parameters_and_learn_bones_checks():
    names = list(inspect.signature(FR.Follower.__init__).parameters)
    assert names[:9] == ['self', 'model_path', 'cameras', 'world', 'assignment', 'capacity', 'single_view', 'learn_bones', 'keywords']
    assert inspect.signature(FR.Follower.__init__).parameters['learn_bones'].default is False
    with pytest.raises(ValueError, match='learn_bones needs world=True'):
        FR.Follower('m', [], learn_bones=True)
    with pytest.raises(ValueError, match='learn_bones must be'):
        FR.Follower('m', [], world=True, learn_bones=1)
    plain = FR.Follower('m', [], world=True)
    assert plain.learn_bones is False and plain.bones is None
    with pytest.raises(ValueError, match='learns no bone lengths'):
        plain.bone_lengths()
    f = FR.Follower('m', [], world=True, single_view='rays', learn_bones=True)
    assert f.learn_bones is True and f.bones is None and f.tracks is None
    for bad in (None, [], [[250.0]], [250.0, -1.0], [250.0, float('nan')], [0.0], [float('inf')]):
        with pytest.raises(ValueError, match='fallback'):
            f.bone_lengths_for(torch.zeros(3, dtype=torch.int32), bad)
    with pytest.raises(ValueError, match='track_index must be an int32 CUDA tensor'):
        f.bone_lengths_for(torch.zeros(3, dtype=torch.int32), [250.0] * 16)
    with pytest.raises(ValueError, match='track_index must be an int32 CUDA tensor'):
        f.bone_lengths_for([0, 1], [250.0] * 16)
    f.bones = 'something'
    f.reset()
    assert f.bones is None and f.tracks is None
    assert list(inspect.signature(FR._follow_world).parameters)[-1] == 'bones'
    assert FR.BoneTable._fields == ('stats', 'ids')
    for bad in (0, 129, True, 2.0):
        with pytest.raises(ValueError, match='capacity'):
            FR.new_bone_table(bad, 16, 'cpu')
    for bad in (0, 65, True):
        with pytest.raises(ValueError, match='n_edges'):
            FR.new_bone_table(8, bad, 'cpu')
    table = FR.new_bone_table(8, 16, 'cpu')
    assert table.stats.shape == (8, 16, 4) and table.stats.dtype == torch.float64 and not table.stats.any()
    assert table.ids.dtype == torch.int32 and table.ids.tolist() == [-1] * 8


def test_bone_length_params_and_track_bone_lengths_checks():
    assert MH.bone_length_params() == (8, 9.0, 1.0, 1.0, 1.0, 1, 1)
    assert MH.bone_length_params(gate=None, debias=False, symmetric=False, cov_scale=0, min_length_mm=0)[1:] == (0.0, 1.0, 0.0, 0.0, 0, 0)
    for bad in (dict(min_count=0), dict(min_count=2.0), dict(min_count=True), dict(gate=-1.0), dict(gate=float('nan')),
                dict(sigma_floor_mm=0.0), dict(sigma_floor_mm=float('inf')), dict(cov_scale=-1.0), dict(min_length_mm=-1.0),
                dict(min_length_mm=float('nan')), dict(debias=1), dict(symmetric='yes')):
        with pytest.raises(ValueError, match=list(bad)[0]):
            MH.bone_length_params(**bad)
        with pytest.raises(ValueError, match=list(bad)[0]):
            MH.track_bone_lengths(None, None, None, None, None, None, None, None, None, **bad)
    assert list(inspect.signature(MH.track_bone_lengths).parameters) == [
        'poses', 'covariance', 'rows', 'starts', 'ids', 'stats', 'bone_ids', 'edges', 'edge_mirror', 'fallback', 'min_count', 'gate',
        'sigma_floor_mm', 'cov_scale', 'min_length_mm', 'debias', 'symmetric']
    assert MH.BoneLengths._fields == ('lengths', 'sigma', 'known')
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match='stats must be'):                   # a host table: there is no CPU path
        MH.track_bone_lengths(None, None, None, None, ids, torch.zeros((4, 16, 4), dtype=torch.float64), ids, np.zeros((16, 2)), np.zeros(16))


def test_placement_refuses_a_tensor_that_is_not_device_bone_lengths():
    """The check of locate_poses_in_frames' bone_lengths: a CPU tensor, or one of the wrong dtype or shape, is refused before any
    launch; host arrays keep their path."""
    cams = object()
    for bad in (torch.full((3, 16), 250.0, dtype=torch.float64), torch.full((3, 16), 250.0), torch.full((16,), 250.0, dtype=torch.float64),
                torch.full((3, 16), 250, dtype=torch.int32)):
        with pytest.raises(ValueError, match='a tensor as bone_lengths must be a contiguous float64 CUDA tensor'):
            FR._placement_targets('bone-lengths', cams, 3, 16, bad, None)
    targets, per_pose, root = FR._placement_targets('bone-lengths', cams, 3, 16, np.full((3, 16), 250.0), None)
    assert isinstance(targets, np.ndarray) and per_pose == 1 and root is None
    assert FR._placement_targets('bone-lengths', cams, 3, 16, [250.0] * 16, None)[1] == 0


def test_locate_poses_refuses_such_a_tensor_before_any_launch(tmp_path):
    from metro_pose3d_amd import ModelSpec, save_model, synth
    from metro_pose3d_amd.camera import Camera
    spec = ModelSpec(50, 32, 'h36m', base_width=8)
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0))
    frame = np.zeros((100, 120, 3), np.uint8)
    boxes = np.array([[10., 10., 40., 60.], [50., 20., 30., 50.]])
    cam = Camera(np.array([[500., 0, 60], [0, 500, 50], [0, 0, 1]]))
    for bad in (torch.full((2, 16), 250.0, dtype=torch.float64), torch.full((2, 16), 250.0), torch.full((16,), 250.0, dtype=torch.float64)):
        with pytest.raises(ValueError, match='a tensor as bone_lengths must be a contiguous float64 CUDA tensor'):
            FR.locate_poses_in_frames(frame, boxes, path, cameras=cam, bone_lengths=bad)
