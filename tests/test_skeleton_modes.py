"""The choice among heat-map modes by bone lengths without a GPU: the fp64 restatement (tests/skeleton_modes_ref.py) on known
answers (the forearm scene of DESIGN.md, K = 1 in closed form, one edge's 2 x 2 table by hand, unknown edges, dead joints),
skeleton_modes.hip's kernel body compiled for the host and walked by a team of one thread and by a team of 64 threads at a
barrier (the same bits), the shapes at its loop boundaries, exact ties, the new C symbol with every refusal, the dispatch of
bound forwards by dry run, and the argument checks of the Python surface that run before any launch.

Bounds (skeleton_modes_ref.compare): choice exact; prob within 1e-9; both logs within 1e-9 max(1, |value|), on the fp64 values
before the one rounding to fp32; coords01_sel exact.  The restatement's two forms agree within 1e-12."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd import heads as MH
from metro_pose3d_amd.joints import skeleton
from tests import heat_modes_ref as MR
from tests import skeleton_modes_ref as SR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: the restatement on known answers -----------------------------------------------------------------------------------------

def scene_modes(sd_mm):
    lg, wrist, wrong = SR.scene_logits(sd_mm)
    voxel, stats = MR.modes(lg, 3, SR.SCENE['depth'], [0, 1, 2], SR.SCENE['k'], SR.SCENE['radius'])
    return voxel, stats, wrist, wrong, lg


@pytest.mark.parametrize('sd_mm', (60.0, 90.0, 140.0))
def test_forearm_scene(sd_mm):
    """The wrist has two peaks, the heavier one is wrong, the mean lies between them; only one is a forearm from the elbow."""
    from tests import heat_moments_ref as HM
    voxel, stats, wrist, wrong, lg = scene_modes(sd_mm)
    a = np.asarray(SR.SCALE)
    lengths = np.asarray([SR.SCENE['bones']])
    res = SR.infer(voxel, stats, lengths, [(0, 1), (1, 2)], SR.SCALE, form='both', sigma_mm=SR.SCENE['sigma_mm'])
    modes_mm = stats[0, 2, :, 2:5] * a
    true_mode = int(np.argmin(np.linalg.norm(modes_mm - wrist, axis=1)))
    heaviest = int(np.argmax(stats[0, 2, :, 0]))
    plain = HM.moments(lg, 3, SR.SCENE['depth'])[0][0, 2] * a
    chosen = modes_mm[res['choice'][0, 2]]
    print(f'sd {sd_mm:.0f} mm: masses {stats[0, 2, :, 0]}, posterior of the true mode {res["prob"][0, 2, true_mode]:.3f}, chosen mean off '
          f'{np.linalg.norm(chosen - wrist):.1f} mm, plain mean off {np.linalg.norm(plain - wrist):.1f} mm, heaviest mode off '
          f'{np.linalg.norm(modes_mm[heaviest] - wrist):.1f} mm, log_evidence {res["log_evidence"][0, 2]:.3f}')
    assert (voxel[0] >= 0).sum() == 4 and heaviest != true_mode, 'one mode per clean joint, two for the wrist, the heavier one wrong'
    assert res['choice'][0, 2] == true_mode and (res['choice'][0, :2] == 0).all()
    assert res['prob'][0, 2, true_mode] >= 0.85
    assert np.linalg.norm(chosen - wrist) <= 20.0 and np.linalg.norm(plain - wrist) > 300.0
    assert np.linalg.norm(modes_mm[heaviest] - wrist) > 600.0


def test_one_mode_per_joint_in_closed_form():
    case = SR.make_case(11, 3, 6, 1, SR.chain(6), missing=0.0, dead=0.0, unknown=0.0)
    res = SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], SR.SCALE, form='both')
    for i in range(3):
        _, _, _, known, lnpsi = SR.potentials(case['voxel'][i], case['stats'][i], case['lengths'][i], case['edges'], SR.SCALE, **SR.DEFAULTS)
        assert known.all() and (lnpsi <= 0).all()
        assert (res['prob'][i] == 1.0).all() and (res['choice'][i] == 0).all()
        assert np.allclose(res['log_evidence'][i], lnpsi.sum(), rtol=0, atol=1e-12 * abs(lnpsi.sum()))
        assert np.allclose(res['log_map'][i], 0.0, atol=1e-12)


def test_one_edge_two_modes_by_hand():
    stats = np.zeros((1, 2, 2, SR.STATS))
    stats[0, :, :, 0] = [[0.6, 0.2], [0.3, 0.5]]
    stats[0, 0, :, 2:5] = [[0.2, 0.2, 0.5], [0.8, 0.2, 0.5]]
    stats[0, 1, :, 2:5] = [[0.2, 0.4, 0.5], [0.8, 0.5, 0.5]]
    voxel = np.zeros((1, 2, 2), np.int32)
    big, sig = 400.0, 30.0
    w = np.array([[0.75, 0.25], [0.375, 0.625]])
    x = stats[0, :, :, 2:5] * np.asarray(SR.SCALE)
    psi = np.array([[np.exp(-(np.linalg.norm(x[1, b] - x[0, a]) - big) ** 2 / (2 * sig ** 2)) for b in range(2)] for a in range(2)])
    table = w[0][:, None] * w[1][None, :] * psi                                   # zero covariances: v = v0, no normaliser
    res = SR.infer(voxel, stats, np.array([[big]]), [(0, 1)], SR.SCALE, form='both', sigma_mm=sig)
    z = table.sum()
    assert np.allclose(res['prob'][0, 0], table.sum(1) / z, atol=1e-14) and np.allclose(res['prob'][0, 1], table.sum(0) / z, atol=1e-14)
    best = np.unravel_index(np.argmax(table), table.shape)
    assert tuple(res['choice'][0]) == best
    assert np.allclose(res['log_evidence'][0], np.log(z), atol=1e-13) and np.allclose(res['log_map'][0], np.log(table.max() / z), atol=1e-13)


def test_an_unknown_edge_splits_the_tree_and_a_dead_joint_cuts_only_its_own_edges():
    case = SR.make_case(5, 1, 5, 2, SR.chain(5), missing=0.0, dead=0.0, unknown=0.0)
    full = SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], SR.SCALE, form='both')
    assert len(set(full['log_evidence'][0])) == 1 and full['log_evidence'][0, 0] < 0
    lengths = case['lengths'].copy()
    lengths[0, 1] = np.nan                                                         # joints {0, 1} and {2, 3, 4}
    split = SR.infer(case['voxel'], case['stats'], lengths, case['edges'], SR.SCALE, form='both')
    assert split['log_evidence'][0, 0] == split['log_evidence'][0, 1] != split['log_evidence'][0, 2] == split['log_evidence'][0, 4]
    lengths[0, 0] = -1.0                                                           # joint 0 alone: the unaries, an evidence of exactly 1
    alone = SR.infer(case['voxel'], case['stats'], lengths, case['edges'], SR.SCALE, form='both')
    w = case['stats'][0, 0, :, 0].astype(np.float64)
    assert alone['log_evidence'][0, 0] == 0.0 and alone['log_evidence'][0, 1] == 0.0
    assert np.array_equal(alone['prob'][0, 0], w / w.sum()) and alone['choice'][0, 0] == int(np.argmax(w))
    assert np.array_equal(alone['prob'][0, 2:], split['prob'][0, 2:])
    voxel = case['voxel'].copy()
    voxel[0, 2] = -1                                                               # joint 2 dead: {0, 1}, {3, 4}
    dead = SR.infer(voxel, case['stats'], case['lengths'], case['edges'], SR.SCALE, form='both')
    assert np.isnan(dead['prob'][0, 2]).all() and dead['choice'][0, 2] == -1 and np.isnan(dead['log_evidence'][0, 2])
    assert np.array_equal(dead['prob'][0, :2], split['prob'][0, :2]) and np.isfinite(dead['prob'][0, 3:]).all()
    assert dead['log_evidence'][0, 3] == dead['log_evidence'][0, 4] < 0


def test_all_lengths_unknown_gives_the_unaries():
    case = SR.make_case(2, 3, 17, 3, [tuple(e) for e in skeleton('h36m').edges], unknown=1.0)
    res = SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], SR.SCALE)
    mass = np.where(case['voxel'] >= 0, case['stats'][..., 0].astype(np.float64), 0.0)
    alive = (case['voxel'] >= 0).any(-1)
    assert np.array_equal(res['choice'][alive], np.argmax(mass, -1)[alive]) and (res['choice'][~alive] == -1).all()
    assert np.array_equal(res['prob'][alive], mass[alive] / mass[alive].sum(-1, keepdims=True))
    assert (res['log_evidence'][alive] == 0.0).all() and np.isnan(res['log_evidence'][~alive]).all()


@pytest.mark.parametrize('dataset,nj,ne', (('h36m', 17, 16), ('many19', 19, 18), ('merged', 19, 18)))
def test_the_three_skeletons_are_trees(dataset, nj, ne):
    sk = skeleton(dataset)
    assert sk.n_out == nj and len(sk.edges) == ne
    assert len(MH.skeleton_edges(sk.edges_array(), nj)) == ne                      # refuses a cycle
    assert len(SR.components(nj, sk.edges, np.ones(ne, bool), np.ones(nj, bool))) == 1


# ---- 2: skeleton_modes.hip compiled for the host ---------------------------------------------------------------------------------

HOST_BODY = '''
#include <pthread.h>
#include <thread>
#include <vector>
struct SkeletonHostTeam {
    int tid, nt;
    pthread_barrier_t* bar;
    void sync() const { if (nt > 1) pthread_barrier_wait(bar); }
};
template <typename OutT>
static void walk_rows(const metro::SkeletonArgs& a, int n, int nt) {
    using namespace metro;
    std::vector<double> lds(sk_lds_bytes(a.J, a.K, a.E) / 8 + 1);                 // exactly the kernel's LDS image
    char* mem = reinterpret_cast<char*>(lds.data());
    if (nt == 1) {
        SkeletonHostTeam team = {0, 1, nullptr};
        for (int i = 0; i < n; ++i) skeleton_walk<OutT>(a, i, mem, team);
        return;
    }
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, (unsigned)nt);
    std::vector<std::thread> lanes;
    for (int t = 0; t < nt; ++t)
        lanes.emplace_back([&a, n, nt, t, mem, &bar] {
            SkeletonHostTeam team = {t, nt, &bar};
            for (int i = 0; i < n; ++i) { skeleton_walk<OutT>(a, i, mem, team); team.sync(); }   // the next row reuses the image
        });
    for (auto& l : lanes) l.join();
    pthread_barrier_destroy(&bar);
}
extern "C" int host_skeleton_modes(const int32_t* voxel, const float* stats, const double* lengths, const float* coords01,
                                   const int32_t* edges, int n_edges, const MetroSkeletonModes* params, int n, int J, int K, int Jhead,
                                   const int32_t* perm, int nt, int wide_out, void* prob, int32_t* choice, void* info, float* sel) {
    using namespace metro;
    SkeletonArgs a = {};
    const char* why = "";
    const int bad = skeleton_schedule(edges, n_edges, J, a.parent, a.parent_edge, &why);
    if (bad >= 0) return -1 - bad;
    a.voxel = voxel; a.stats = stats; a.lengths = lengths; a.coords01 = coords01;
    a.prob = prob; a.choice = choice; a.info = info; a.coords01_sel = sel;
    a.J = J; a.K = K; a.E = n_edges; a.Jhead = Jhead; a.p = *params;
    for (int j = 0; j < J; ++j) a.perm[j] = (unsigned char)perm[j];
    for (int e = 0; e < n_edges; ++e) { a.edge[e][0] = (unsigned char)edges[2 * e]; a.edge[e][1] = (unsigned char)edges[2 * e + 1]; }
    if (sk_lds_bytes(J, K, n_edges) > (size_t)SK_LDS_MAX) return -1000;
    if (wide_out) walk_rows<double>(a, n, nt); else walk_rows<float>(a, n, nt);
    return 0;
}
'''


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return compile_for_host(tmp_path_factory.mktemp('skeleton_modes_host'), 'skeleton_modes_host', ['skeleton_modes.hip'], HOST_BODY)


def run_host(host, case, nt=1, wide=True, with_sel=True, **options):
    params = MH.skeleton_mode_params(SR.SCALE, **dict(SR.DEFAULTS, **options))
    rows, nj, k = case['rows'], case['nj'], case['k']
    voxel, stats = np.ascontiguousarray(case['voxel'], np.int32), np.ascontiguousarray(case['stats'], np.float32)
    lengths, coords01 = np.ascontiguousarray(case['lengths'], np.float64), np.ascontiguousarray(case['coords01'], np.float32)
    edges = np.ascontiguousarray(np.asarray(case['edges'], np.int32).reshape(-1, 2))
    perm = np.asarray(case['perm'], np.int32)
    out_t = np.float64 if wide else np.float32
    prob, info = np.full((rows, nj, k), 7.0, out_t), np.full((rows, nj, 2), 7.0, out_t)
    choice, sel = np.full((rows, nj), 7, np.int32), np.full((rows, case['n_head'], 3), 7.0, np.float32)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    st = host.host_skeleton_modes(p(voxel), p(stats), p(lengths), p(coords01), p(edges), len(edges), C.byref(params), rows, nj, k,
                                  case['n_head'], p(perm), nt, int(wide), p(prob), p(choice), p(info), p(sel) if with_sel else None)
    assert st == 0, st
    return dict(prob=prob, choice=choice, info=info, sel=sel if with_sel else None)


def hold(host, case, what, **options):
    ref = SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], SR.SCALE, form='both', **options)
    got = run_host(host, case, **options)
    SR.compare(got, case, ref, what)
    return got, ref


def test_host_code_on_the_forearm_scene(host):
    voxel, stats, wrist, _, lg = scene_modes(90.0)
    case = dict(voxel=voxel, stats=stats.astype(np.float32), lengths=np.asarray([SR.SCENE['bones']]), edges=[(0, 1), (1, 2)],
                coords01=np.zeros((1, 3, 3), np.float32), perm=[0, 1, 2], k=2, nj=3, n_head=3, rows=1)
    got, ref = hold(host, case, 'forearm scene')
    true_mode = int(np.argmin(np.linalg.norm(stats[0, 2, :, 2:5] * np.asarray(SR.SCALE) - wrist, axis=1)))
    assert got['choice'][0, 2] == true_mode and got['prob'][0, 2, true_mode] >= 0.85
    assert np.array_equal(got['sel'][0, 2], case['stats'][0, 2, true_mode, 2:5])


SKELETONS = {name: [tuple(e) for e in skeleton(name).edges] for name in ('h36m', 'many19', 'merged')}
SHAPES = [
    # (id, rows, Jout, K, edges)
    ('one-joint', 2, 1, 2, []),
    ('two-joints-no-edge', 2, 2, 2, []),
    ('two-joints', 65, 2, 8, [(1, 0)]),
    ('h36m-k1', 2, 17, 1, SKELETONS['h36m']),
    ('h36m-k2', 65, 17, 2, SKELETONS['h36m']),
    ('h36m-k8', 2, 17, 8, SKELETONS['h36m']),
    ('many19-k2', 2, 19, 2, SKELETONS['many19']),
    ('merged-k8', 1, 19, 8, SKELETONS['merged']),
    ('h36m-no-edge', 1, 17, 2, []),
    ('h36m-one-edge', 2, 17, 2, SKELETONS['h36m'][5:6]),
    ('chain-64-k2', 2, 64, 2, SR.chain(64)),
    ('chain-64-k8', 1, 64, 8, SR.chain(64)),
    ('chain-64-reversed', 1, 64, 2, [(j + 1, j) for j in range(63)][::-1]),
    ('star-63-k2', 2, 64, 2, SR.star(64)),
    ('star-63-k8', 1, 64, 8, SR.star(64)),
    ('star-63-centre-last', 1, 64, 2, [(63, j) for j in range(63)]),
    ('forest-64', 2, 64, 3, None),                                                  # a random forest of 40 edges
]


def shape_case(name, rows, nj, k, edges, **kw):
    seed = [len(name), rows, nj, k]
    if edges is None:
        edges = SR.random_tree(np.random.default_rng(seed), nj, 40)
    return SR.make_case(seed, rows, nj, k, edges, n_head=min(64, nj + 3), **kw)


@pytest.mark.parametrize('name,rows,nj,k,edges', SHAPES, ids=[s[0] for s in SHAPES])
def test_host_code_over_shapes(host, name, rows, nj, k, edges):
    hold(host, shape_case(name, rows, nj, k, edges), name)


@pytest.mark.parametrize('name,rows,nj,k,edges', [s for s in SHAPES if s[0] in ('h36m-k2', 'chain-64-k2', 'star-63-k2', 'forest-64')],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_host_code_with_nothing_missing_and_with_much_missing(host, name, rows, nj, k, edges):
    hold(host, shape_case(name, min(rows, 3), nj, k, edges, missing=0.0, dead=0.0, unknown=0.0), name + ' complete')
    hold(host, shape_case(name, min(rows, 3), nj, k, edges, missing=0.4, dead=0.2, unknown=0.4), name + ' sparse')


@pytest.mark.parametrize('options', (dict(sigma_rel=0.1), dict(cov_scale=0.0), dict(sigma_mm=5.0, cov_scale=3.0), dict(min_length_mm=3000.0)),
                         ids=('sigma-rel', 'no-cov', 'sharp', 'all-below-min-length'))
def test_host_code_over_options(host, options):
    hold(host, shape_case('options', 3, 17, 3, SKELETONS['h36m']), str(options), **options)


def test_host_code_with_random_trees_re_rooted(host):
    """Random forests in random edge order and orientation, many unknown edges: every cut leaves a component whose lowest joint is
    rarely the schedule's root, so the re-rooting walk runs on most of them."""
    for seed in range(6):
        rng = np.random.default_rng(seed)
        nj = int(rng.integers(3, 40))
        case = SR.make_case(seed + 100, 3, nj, 3, SR.random_tree(rng, nj), unknown=0.3, n_head=nj)
        hold(host, case, f'random tree {seed} ({nj} joints)')


def test_non_finite_stats_are_absent_modes_and_touch_nothing_else(host):
    case = shape_case('poison', 2, 17, 3, SKELETONS['h36m'], missing=0.0, dead=0.0, unknown=0.0)
    clean = run_host(host, case)
    bad = dict(case, stats=case['stats'].copy())
    bad['stats'][0, 4, 1, 3] = np.nan                                              # a coordinate
    bad['stats'][0, 9, :, 0] = [np.inf, np.nan, -1.0]                              # every mass of joint 9: dead
    bad['stats'][0, 2, 0, 7] = np.inf                                              # a covariance word
    got, ref = hold(host, bad, 'poisoned')
    assert got['prob'][0, 4, 1] == 0 and got['prob'][0, 2, 0] == 0 and np.isnan(got['prob'][0, 9]).all() and got['choice'][0, 9] == -1
    assert np.isfinite(np.delete(got['prob'][0], 9, axis=0)).all()
    for key in ('prob', 'choice', 'info', 'sel'):
        assert np.array_equal(got[key][1], clean[key][1]), key                     # the other crop keeps its bits
    assert np.array_equal(got['sel'][0, case['perm'][9]], case['coords01'][0, case['perm'][9]]), 'a dead joint keeps the plain mean'


def test_rows_beyond_n_and_an_absent_sel_output(host):
    case = shape_case('partial', 3, 17, 2, SKELETONS['h36m'])
    full = run_host(host, case)
    part = run_host(host, dict(case, rows=2))                                       # buffers of 2 rows: the third is never touched
    for key in ('prob', 'choice', 'info', 'sel'):
        assert np.array_equal(part[key], full[key][:2], equal_nan=True), key
    none = run_host(host, case, with_sel=False)
    assert np.array_equal(none['prob'], full['prob'], equal_nan=True) and np.array_equal(none['choice'], full['choice'])
    head_only = [h for h in range(case['n_head']) if h not in case['perm']]
    assert head_only and np.array_equal(full['sel'][:, head_only], case['coords01'][:, head_only]), 'head joints outside the output order'


def tie_case(kind):
    """'twin': the second mode of every joint is a copy of the first, so all 2^17 assignments tie in every bit.  'mirror': it is
    the first mirrored in x (x on a grid of 2^-10, so 1 - x is exact in fp32; cov xy and xz change sign with it): the all-first
    and the all-second assignment tie in real arithmetic, and to within rounding in fp64."""
    case = SR.make_case(77, 3, 17, 2, SKELETONS['h36m'], missing=0.0, dead=0.0, unknown=0.0)
    st = case['stats']
    st[:, :, 0, 2] = np.round(st[:, :, 0, 2] * 1024) / 1024
    st[:, :, 1] = st[:, :, 0]
    if kind == 'mirror':
        st[:, :, 1, 2] = 1.0 - st[:, :, 0, 2]
        st[:, :, 1, 8:10] = -st[:, :, 0, 8:10]
    return case


@pytest.mark.parametrize('kind', ('twin', 'mirror'))
def test_exact_ties(host, kind):
    """Held to what every optimum shares: the returned assignment's log-probability is the maximum within 1e-9, and two runs are
    identical.  Where the tie is exact in every bit ('twin') the lowest index wins at every step: mode 0 everywhere."""
    case = tie_case(kind)
    st = case['stats']
    first, again = run_host(host, case), run_host(host, case)
    for key in ('prob', 'choice', 'info', 'sel'):
        assert np.array_equal(first[key], again[key]), key
    ref = SR.infer(case['voxel'], st, case['lengths'], case['edges'], SR.SCALE)
    assert (ref['gap'] < SR.MIN_GAP).all(), 'the case must tie'
    for i in range(case['rows']):
        row = lambda choice: SR.assignment_log_prob(choice, case['voxel'][i], st[i], case['lengths'][i], case['edges'], SR.SCALE)
        got_lp = row(first['choice'][i]) - ref['log_evidence'][i]
        assert np.abs(got_lp - ref['log_map'][i]).max() <= 1e-9, np.abs(got_lp - ref['log_map'][i]).max()
        assert np.abs(first['info'][i, :, 1] - ref['log_map'][i]).max() <= 1e-9
    if kind == 'twin':
        assert (first['choice'] == 0).all()
        assert np.abs(first['prob'] - 0.5).max() <= 1e-9


@pytest.mark.parametrize('name', ('h36m-k2', 'chain-64-k8', 'star-63-k2', 'forest-64', 'two-joints'))
def test_a_team_of_one_and_a_team_of_64_give_the_same_bits(host, name):
    shape = next(s for s in SHAPES if s[0] == name)
    case = shape_case(*shape[:2], *shape[2:])
    case = dict(case, rows=min(case['rows'], 3))
    for wide in (True, False):
        one, many = run_host(host, case, 1, wide), run_host(host, case, 64, wide)
        for key in ('prob', 'choice', 'info', 'sel'):
            assert np.array_equal(one[key][:case['rows']], many[key][:case['rows']], equal_nan=True), (name, key, wide)


def test_fp32_outputs_are_the_fp64_ones_rounded_once(host):
    case = shape_case('h36m-k2', 3, 17, 2, SKELETONS['h36m'])
    wide, narrow = run_host(host, case, wide=True), run_host(host, case, wide=False)
    assert np.array_equal(wide['prob'].astype(np.float32), narrow['prob'], equal_nan=True)
    assert np.array_equal(wide['info'].astype(np.float32), narrow['info'], equal_nan=True)
    assert np.array_equal(wide['choice'], narrow['choice']) and np.array_equal(wide['sel'], narrow['sel'])


# ---- 3: the Python surface -------------------------------------------------------------------------------------------------------

def test_skeleton_mode_params_validates_the_keywords():
    p = MH.skeleton_mode_params(SR.SCALE)
    assert (tuple(p.scale_mm), p.sigma_mm, p.sigma_rel, p.cov_scale, p.min_length_mm) == (SR.SCALE, 20.0, 0.0, 1.0, 1.0)
    assert 'design choices, not measurements' in MH.skeleton_mode_params.__doc__
    for kw, word in ((dict(sigma_mm=0.0), 'sigma_mm'), (dict(sigma_mm=float('nan')), 'sigma_mm'), (dict(sigma_rel=-0.1), 'sigma_rel'),
                     (dict(cov_scale=float('inf')), 'cov_scale'), (dict(min_length_mm=-1.0), 'min_length_mm'), (dict(sigma_mm=True), 'sigma_mm')):
        with pytest.raises(ValueError, match=word):
            MH.skeleton_mode_params(SR.SCALE, **kw)
    for scale in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, float('nan'), 1.0), 5.0):
        with pytest.raises(ValueError, match='scale_mm'):
            MH.skeleton_mode_params(scale)


def test_skeleton_edges_refuses_what_is_no_forest():
    assert MH.skeleton_edges([], 3).shape == (0, 2)
    assert MH.skeleton_edges([(0, 1), (2, 1)], 3).dtype == np.int32
    for edges, word in (([(0, 1), (1, 2), (2, 0)], 'edge 2 .* cycle'), ([(0, 0)], 'edge 0'), ([(0, 3)], 'edge 0'), ([(0, 1), (1, 0)], 'edge 1 .* cycle'),
                        (SR.chain(65), 'E <= 63'), ([(0.5, 1.0)], 'integers')):
        with pytest.raises(ValueError, match=word):
            MH.skeleton_edges(edges, 65 if len(edges) > 3 else 3)


def test_exports():
    import metro_pose3d_amd as M
    from metro_pose3d_amd import inference as INF
    from metro_pose3d_amd.engine import Engine
    assert M.estimate_pose_skeleton is INF.estimate_pose_skeleton and M.SkeletonModes is INF.SkeletonModes
    assert 'estimate_pose_skeleton' in M.__all__ and 'SkeletonModes' in M.__all__
    assert INF.SkeletonModes._fields == ('poses', 'choice', 'prob', 'log_evidence', 'log_map')
    sig = inspect.signature(Engine.forward_skeleton_modes).parameters
    assert [sig[n].default for n in ('k', 'radius', 'edges', 'sigma_mm', 'sigma_rel', 'cov_scale', 'min_length_mm')] == [2, 1, None, 20.0, 0.0, 1.0, 1.0]
    with pytest.raises(ValueError, match='shard'):
        INF.estimate_pose_skeleton(np.zeros((1, 256, 256, 3), np.float32), 'no-such-model', np.ones(16), shard=True)


def test_the_frames_call_checks_before_any_launch():
    import metro_pose3d_amd as M
    from metro_pose3d_amd import frames as FR
    assert M.locate_skeleton_poses_in_frames is FR.locate_skeleton_poses_in_frames and M.SkeletonFramePoses is FR.SkeletonFramePoses
    assert FR.SkeletonFramePoses._fields == ('plain', 'selected', 'choice', 'prob', 'log_evidence', 'log_map')
    assert callable(FR.Follower.locate_skeleton)
    frame = [np.zeros((64, 64, 3), np.uint8)]
    boxes = np.array([[8.0, 8, 32, 32]])
    for kw, word in ((dict(k=0), 'k must be'), (dict(k=9), 'k must be'), (dict(radius=-1), 'radius'), (dict(sigma_mm=0.0), 'sigma_mm'),
                     (dict(cov_scale=-1.0), 'cov_scale'), (dict(views=0), 'views')):
        with pytest.raises(ValueError, match=word):
            FR.locate_skeleton_poses_in_frames(frame, boxes, 'no-such-model', None, np.ones(16), **kw)


def test_a_flipped_view_reads_the_mirror_columns():
    from metro_pose3d_amd import frames as FR
    for name in ('h36m', 'many19', 'merged'):
        sk = skeleton(name)
        em = np.asarray(sk.edge_mirror())
        cols = FR._view_edge_columns(FR.view_set([(0.0, 1.0, False), (5.0, 1.0, True)]), sk)
        assert cols.shape == (2, len(sk.edges)) and np.array_equal(cols[0], np.arange(len(em)))
        assert np.array_equal(cols[1], np.where(em >= 0, em, np.arange(len(em)))) and not np.array_equal(cols[1], cols[0])
        assert np.array_equal(cols[1][cols[1]], cols[0]), 'mirroring twice is the identity'
        assert np.array_equal(FR._view_edge_columns(FR.view_set(1), sk), cols[:1])


def test_skeleton_to_metric_roots_at_the_chosen_root():
    import torch
    from metro_pose3d_amd import inference as INF
    rng = np.random.default_rng(0)
    for dataset in ('h36m', 'merged'):
        spec = ModelSpec(50, 16, dataset)
        sk = spec.skeleton
        sel = rng.uniform(0, 1, (2, sk.n_head, 3)).astype(np.float32)
        a, b = (np.asarray(v) for v in INF._metric_map(spec))
        mm = sel.astype(np.float64) * a + b
        want = (mm[:, list(sk.permutation)] - mm[:, -1:]).astype(np.float32)
        assert np.array_equal(INF.skeleton_to_metric(spec, torch.from_numpy(sel)).numpy(), want)


# ---- 4: the C surface ------------------------------------------------------------------------------------------------------------

def test_symbol_in_header_bindings_and_library():
    header = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    proto = re.search(r'int\s+metro_plan_bind_skeleton_modes\(([^;]*)\);', header).group(1)
    assert 'stream' not in proto and 'scratch' not in proto, 'a bind entry takes no stream (no new launching entry) and no scratch'
    assert len(proto.split(',')) == len(_lib.SIGNATURES['metro_plan_bind_skeleton_modes'][1]) == 13
    lib = _lib.load()
    assert hasattr(lib, 'metro_plan_bind_skeleton_modes')
    assert re.search(r'#define METRO_ABI_VERSION 8\b', header) and lib.metro_abi_version() == 8
    assert C.sizeof(_lib.MetroSkeletonModes) == 56 and _lib.MetroSkeletonModes.sigma_mm.offset == 24
    for word in ('design choices, not measurements', 'can only choose among the modes', 'a skeleton with a cycle is refused'):
        assert word in header, word
    from metro_pose3d_amd import build
    assert 'skeleton_modes.hip' in build.SOURCES
    assert 'metro_plan_bind_skeleton_modes' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def _plan(lib, spec, precision=1, max_batch=4):
    plan = C.c_void_p()
    cs = spec.to_c(precision)
    _lib.check(lib.metro_plan_create(C.byref(cs), max_batch, C.byref(plan)), 'metro_plan_create')
    return plan


NAMES = ('voxel', 'stats', 'lengths', 'prob', 'choice', 'info', 'sel')
H36M_EDGES = np.ascontiguousarray(skeleton('h36m').edges_array(), np.int32)


def _binder(lib, plan):
    ptrs = {name: C.c_void_p(4096 * (i + 1)) for i, name in enumerate(NAMES)}     # nothing is dereferenced at bind time
    good = MH.skeleton_mode_params(SR.SCALE)

    def bind(params=good, k=2, edges=H36M_EDGES, n_edges=None, max_n=4, **swap):
        p = dict(ptrs, **swap)
        e = np.ascontiguousarray(edges, np.int32) if edges is not None else None
        n_edges = (len(e) if e is not None else 0) if n_edges is None else n_edges
        return lib.metro_plan_bind_skeleton_modes(plan, p['voxel'], p['stats'], k, p['lengths'], e.ctypes.data_as(C.c_void_p) if e is not None and e.size else None,
                                                  n_edges, C.byref(params) if params is not None else None, p['prob'], p['choice'],
                                                  p['info'], p['sel'], max_n)
    return bind


def _unbind(lib, plan):
    return lib.metro_plan_bind_skeleton_modes(plan, None, None, 0, None, None, 0, None, None, None, None, None, 0)


def test_bind_refusals_one_by_one():
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8))
    bind = _binder(lib, plan)
    try:
        assert bind() == 0 and bind(sel=None) == 0, 'with coords01_sel, and without'
        assert bind(edges=None) == 0, 'no edges: the unaries'
        for name in NAMES[:-1]:
            assert bind(**{name: None}) == -1 and b'go together' in lib.metro_last_error(), name
        assert bind(params=None) == -1 and b'go together' in lib.metro_last_error()
        for name in NAMES:
            assert bind(**{name: C.c_void_p(4096 * 20 + 2)}) == -1 and b'aligned' in lib.metro_last_error(), name
        assert bind(lengths=C.c_void_p(4096 * 20 + 4)) == -1 and b'8-byte' in lib.metro_last_error()
        for max_n in (0, 5, -1):
            assert bind(max_n=max_n) == -1 and b'max_n' in lib.metro_last_error()
        for k in (0, 9, -1):
            assert bind(k=k) == -1 and b'k ' in lib.metro_last_error()
        assert bind(n_edges=-1) == -1 and b'n_edges' in lib.metro_last_error()
        assert bind(n_edges=64) == -1 and b'n_edges' in lib.metro_last_error()
        assert bind(edges=None, n_edges=3) == -1 and b'h_edges' in lib.metro_last_error()
        for edges, word in (([(0, 1), (1, 17)], b'edge 1 (1, 17)'), ([(0, 1), (-1, 2)], b'edge 1 (-1, 2)'), ([(3, 3)], b'edge 0 (3, 3)'),
                            ([(0, 1), (1, 2), (2, 0)], b'edge 2 (2, 0) closes a cycle'), ([(0, 1), (1, 0)], b'edge 1 (1, 0) closes a cycle')):
            assert bind(edges=edges) == -1 and word in lib.metro_last_error(), (edges, lib.metro_last_error())
        for field, value in (('sigma_mm', 0.0), ('sigma_mm', float('inf')), ('sigma_mm', float('nan')), ('sigma_rel', -1.0),
                             ('sigma_rel', float('nan')), ('cov_scale', -1.0), ('cov_scale', float('inf')), ('min_length_mm', -1.0),
                             ('min_length_mm', float('nan'))):
            p = MH.skeleton_mode_params(SR.SCALE)
            setattr(p, field, value)
            assert bind(params=p) == -1 and field.encode() in lib.metro_last_error(), (field, value, lib.metro_last_error())
        for i, value in ((0, 0.0), (1, float('inf')), (2, float('nan')), (2, -3.0)):
            p = MH.skeleton_mode_params(SR.SCALE)
            p.scale_mm[i] = value
            assert bind(params=p) == -1 and f'scale_mm[{i}]'.encode() in lib.metro_last_error(), (i, value)
        assert _unbind(lib, plan) == 0 and _unbind(lib, plan) == 0
        # all pointers NULL but a size left: not the unbind call
        assert lib.metro_plan_bind_skeleton_modes(plan, None, None, 0, None, None, 0, None, None, None, None, None, 1) == -1
        assert lib.metro_plan_bind_skeleton_modes(plan, None, None, 2, None, None, 0, None, None, None, None, None, 0) == -1
    finally:
        lib.metro_plan_destroy(plan)


def test_forward_refusals_before_any_launch():
    """n > max_n, and a forward entry without a coords01 output while coords01_sel is bound: METRO_ERR_INVALID_ARG from the checks
    that run before the first launch (the parameters are a fake blob; nothing is enqueued)."""
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8), max_batch=4)
    bind = _binder(lib, plan)
    fake = C.c_void_p(1 << 20)
    try:
        assert lib.metro_plan_bind_params(plan, fake) == 0
        assert bind(max_n=2) == 0
        assert lib.metro_forward_coords01(plan, fake, 3, fake, fake, fake, None) == -1 and b'metro_plan_bind_skeleton_modes' in lib.metro_last_error()
        assert lib.metro_forward(plan, fake, 2, fake, fake, None) == -1 and b'coords01' in lib.metro_last_error()
        assert lib.metro_forward_moments(plan, fake, 0, 2, fake, None, None, None, None, fake, None) == -1 and b'coords01' in lib.metro_last_error()
    finally:
        lib.metro_plan_destroy(plan)


def _dry_ids(lib, plan, n, coords01=True):
    dry = C.c_void_p(4096)
    _lib.check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        _lib.check(lib.metro_forward_moments(plan, dry, 0, int(n), dry, dry if coords01 else None, dry, dry, dry, dry, None),
                   'metro_forward_moments (dry run)')
        return lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)


@pytest.mark.parametrize('precision', ('f16', 'f32', 'f64'))
def test_dispatch_of_bound_forwards_by_dry_run(precision):
    """Bound, skeleton_modes follows heat_modes (or the plan's own last launch where modes are not bound) and comes before the
    other bound launches; one instantiation for every precision; without coords01_sel no coords01 output is needed; unbound, the
    plan's own list again."""
    from metro_pose3d_amd.engine import Engine
    from tests.test_gpu_heat_modes import MODES_IDS as MODE_IDS
    lib = _lib.load()
    eng = Engine(ModelSpec(50, 16, 'h36m'), None, precision, max_batch=64)
    plan, dry = eng._plan, C.c_void_p(4096)
    bind = _binder(lib, plan)
    _lib.check(lib.metro_plan_bind_params(plan, dry), 'metro_plan_bind_params')
    try:
        for n in (1, 3, 64):
            plain = _dry_ids(lib, plan, n)
            assert 'skeleton_modes' not in plain
            assert bind(max_n=64) == 0
            assert _dry_ids(lib, plan, n) == plain + ' & skeleton_modes', n
            assert bind(max_n=64, sel=None) == 0
            assert _dry_ids(lib, plan, n, coords01=False) == _dry_ids(lib, plan, n) == plain + ' & skeleton_modes', n
            _lib.check(lib.metro_plan_bind_modes(plan, dry, dry, dry, 64, 2, 1), 'bind')
            _lib.check(lib.metro_plan_bind_prior(plan, dry, dry, dry, 64), 'bind')
            ids = _dry_ids(lib, plan, n).split(' & ')
            assert ids[-3] == MODE_IDS[precision] and ids[-2] == 'skeleton_modes' and ids[-1].startswith('heat_posterior'), ids[-3:]
            _lib.check(lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0), 'unbind')
            _lib.check(lib.metro_plan_bind_prior(plan, None, None, None, 0), 'unbind')
            assert _unbind(lib, plan) == 0
            assert _dry_ids(lib, plan, n) == plain, 'unbind restores the launch list'
    finally:
        lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0)
        lib.metro_plan_bind_prior(plan, None, None, None, 0)
        _unbind(lib, plan)
        eng.close()
