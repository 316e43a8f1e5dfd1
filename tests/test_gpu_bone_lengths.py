"""metro_track_bone_lengths, frames.Follower(learn_bones=True) and locate_poses_in_frames' device bone lengths on the MI355X: the
launch against its fp64 restatement (tests/bone_lengths_ref.py) on the cases and bounds of tests/test_bone_lengths.py, cut streams
bit for bit, the read-out alone, the follower's table against heads.track_bone_lengths composed by hand, and placement with a
CUDA tensor of bone lengths against the same call with its host copy.  Every GPU step runs once."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import frames as FR, heads as MH
from tests import bone_lengths_ref as BL

gpu = pytest.mark.gpu


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _launch(case, cuda):
    """Every call of the case through heads.track_bone_lengths on a fresh table -> ([stats after each call], bone_ids,
    (lengths, sigma, known) of the last), NumPy."""
    table = FR.new_bone_table(case['T'], len(case['edges']), cuda)
    after, out = [], None
    with torch.cuda.device(cuda):
        for call in case['calls']:
            poses = None if call['poses'] is None else _up(call['poses'], cuda)
            cov = None if call['cov'] is None else _up(call['cov'], cuda)
            out = MH.track_bone_lengths(poses, cov, call['rows'], call['starts'], _up(call['ids'], cuda), table.stats, table.ids,
                                        case['edges'], case['mirror'], case['fallback'], **case['params'])
            after.append(table.stats.cpu().numpy())
    assert [t.dtype for t in out] == [torch.float64, torch.float64, torch.uint8]
    return after, table.ids.cpu().numpy(), tuple(t.cpu().numpy() for t in out)


CASES = {'isotropic': BL.isotropic_case, 'arm-pooled': lambda: BL.arm_case(True)[0], 'arm-alone': lambda: BL.arm_case(False)[0],
         'outlier-late': lambda: BL.outlier_case(10)[0], 'outlier-early': lambda: BL.outlier_case(3)[0],
         'forget': lambda: BL.forget_case(True), 'accumulate': lambda: BL.forget_case(False), 'bias': lambda: BL.bias_case(0),
         **{name: (lambda name=name: BL.shape_case(name)) for name in BL.SHAPES}}


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_launch_matches_the_restatement(cuda, name):
    """count, rejected and known exact; S0, S1, lengths and sigma within 1e-9 relative: fp64 rounding over at most 2e4 terms."""
    case = CASES[name]()
    after, bone_ids, out = _launch(case, cuda)
    worst = BL.compare(after[-1], out, case, name)
    assert np.array_equal(bone_ids, case['calls'][-1]['ids'])
    print(f"{name}: T {case['T']}, E {len(case['edges'])}, {int(after[-1][..., 2].sum())} samples, {int(after[-1][..., 3].sum())} rejected, "
          f'{int(out[2].sum())} of {out[2].size} known, worst relative deviation {worst:.2e}')


@gpu
def test_a_cut_stream_leaves_the_same_stats_bit_for_bit(cuda):
    whole = _launch(BL.cut_case(None), cuda)
    assert (whole[0][-1][..., 2] > 0).any()
    for steps in BL.CUTS[1:]:
        cut = _launch(BL.cut_case(steps), cuda)
        assert np.array_equal(cut[0][-1].view(np.int64), whole[0][-1].view(np.int64)), steps
        for a, b in zip(cut[2], whole[2]):
            assert np.array_equal(a, b, equal_nan=True), steps


@gpu
def test_no_rows_is_a_read_out_alone(cuda):
    """n_rows = 0: the launch still resets the slot whose id changed and reads every slot out; stats it keeps are untouched."""
    case = BL.forget_case(False)
    quiet = dict(case['calls'][1], poses=None, cov=None, rows=np.zeros(0, np.int32), ids=case['calls'][0]['ids'] + np.array([0, 9], np.int32))
    case['calls'] = [case['calls'][0], quiet]
    after, bone_ids, (lengths, sigma, known) = _launch(case, cuda)
    assert np.array_equal(after[1][0].view(np.int64), after[0][0].view(np.int64)) and (after[1][1] == 0).all() and (after[0][1] != 0).any()
    assert known[0].any() and not known[1].any() and np.array_equal(lengths[1], case['fallback']) and np.isnan(sigma[1]).all()
    assert np.array_equal(bone_ids, quiet['ids'])
    BL.compare(after[-1], (lengths, sigma, known), case, 'read-out alone')
    # rows listed but no pose rows at all: the same
    table = FR.new_bone_table(2, 16, cuda)
    with torch.cuda.device(cuda):
        out = MH.track_bone_lengths(torch.zeros((0, 17, 3), device=cuda), None, [0, 1], [0, 1, 2], _up(np.array([4, 5], np.int32), cuda),
                                    table.stats, table.ids, case['edges'], case['mirror'])
    assert table.ids.tolist() == [4, 5] and not table.stats.any() and torch.isnan(out.lengths).all() and not out.known.any()


COV_SCALE = 1e-4


def _csr_by_hand(track_index, person_step, n_tracks):
    """The CSR the association wrote, rebuilt from what the call returned: slot t owns its persons in time order."""
    ti, step = track_index.cpu().numpy(), person_step.cpu().numpy()
    groups = [np.flatnonzero(ti == t) for t in range(n_tracks)]
    groups = [g[np.argsort(step[g], kind='stable')] for g in groups]
    return np.concatenate(groups).astype(np.int32), np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)


@gpu
@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_follower_learns_what_the_launch_composed_by_hand_learns(cuda, tmp_path, precision):
    """A synthetic model's poses mean nothing, so this holds composition and bits.  Two calls (the two exposures of the 3-camera
    rig): .bones.stats is heads.track_bone_lengths on the world poses, covariance, track_index and table ids the call returned,
    and every output is what the same stream gives without learn_bones.  Then the first exposure eight more times at later
    stamps (the same poses: its tracks continue), so that a bone can reach its min_count rows; what was learned is held to the
    restatement run on the arrays the calls returned.
    The synthetic model's heat maps are flat: its joints have a standard deviation near a metre, larger than the bones it places
    (16 to 280 mm), and at cov_scale = 1 every debiased length is <= 0 and rightly skipped.  cov_scale = 1e-4 (the follower's own
    keyword, the filter's too) brings that to about 10 mm, the regime the estimator is for."""
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_single_view import _same
    from tests.test_gpu_world_follow import _rig
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision=precision, capacity=8, cov_scale=COV_SCALE)
    learn = FR.Follower(path, cams[:3], world=True, single_view='rays', learn_bones=True, **kw)
    plain = FR.Follower(path, cams[:3], world=True, single_view='rays', **kw)
    by_hand, ref = FR.new_bone_table(8, len(sk.edges), cuda), BL.new_table(8, len(sk.edges))
    for k, t in enumerate([0, 1] + [0] * 8):
        sel = fi // 3 == t
        args = (frames[3 * t:3 * t + 3], boxes[sel], fi[sel] - 3 * t, [0.125 * k] * 3)
        got = learn.follow(*args)
        if k < 2:
            want = plain.follow(*args)
            for name in FR.FollowedRigPoses._fields:
                a, b = getattr(got, name), getattr(want, name)
                assert _same(tuple(a) if isinstance(a, tuple) else a, tuple(b) if isinstance(b, tuple) else b), (k, name)
        rows, starts = _csr_by_hand(got.track_index, got.person_step, 8)
        with torch.cuda.device(cuda):
            MH.track_bone_lengths(got.world.poses, got.world_covariance, rows, starts, got.tracks.ids, by_hand.stats, by_hand.ids,
                                  sk.edges, sk.edge_mirror(), cov_scale=COV_SCALE)
        assert torch.equal(learn.bones.stats.view(torch.int64), by_hand.stats.view(torch.int64)), k
        assert torch.equal(learn.bones.ids, by_hand.ids) and torch.equal(learn.bones.ids, got.tracks.ids), k
        BL.update(ref, got.world.poses.cpu().numpy(), got.world_covariance.cpu().numpy(), rows, starts, got.tracks.ids.cpu().numpy(),
                  sk.edges, cov_scale=COV_SCALE)
    assert ref['samples'] and sum(map(len, ref['samples'].values())) > 0, 'the stream teaches something'
    # what was learned, against the restatement on the arrays the calls returned
    stats, want_stats = learn.bones.stats.cpu().numpy(), BL.stats(ref)
    assert np.array_equal(stats[..., 2:], want_stats[..., 2:])
    assert np.allclose(stats[..., :2], want_stats[..., :2], rtol=1e-9, atol=0.0)
    want_lengths, _, want_known = BL.read_out(ref, sk.edge_mirror())
    read = learn.bone_lengths()
    assert np.array_equal(read.known.cpu().numpy(), want_known) and torch.isnan(read.lengths[read.known == 0]).all()
    assert np.allclose(read.lengths.cpu().numpy()[want_known == 1], want_lengths[want_known == 1], rtol=1e-9, atol=0.0)
    # the learned lengths per predicted box, on the device
    fallback = np.linspace(200.0, 400.0, len(sk.edges))
    predicted = learn.predict(FR.frame_sizes(frames[:3]), [1.3] * 3)
    slots = torch.cat([predicted.track_index, torch.tensor([-1, 8, 2], dtype=torch.int32, device=cuda)])
    assert predicted.n_predicted > 0
    lengths = learn.bone_lengths_for(slots, fallback)
    assert lengths.dtype == torch.float64 and tuple(lengths.shape) == (len(slots), len(sk.edges)) and lengths.is_contiguous()
    assert torch.isfinite(lengths).all() and (lengths > 0).all()
    filled = learn.bone_lengths(fallback)
    table = torch.cat([filled.lengths, _up(fallback, cuda)[None]])
    index = torch.where((slots >= 0) & (slots < 8), slots, torch.full_like(slots, 8)).long()
    assert torch.equal(lengths, table[index]) and torch.equal(lengths[-3], _up(fallback, cuda)) and torch.equal(lengths[-2], lengths[-3])
    assert torch.equal(filled.lengths[read.known == 1], read.lengths[read.known == 1]) and torch.equal(filled.known, read.known)
    own = (lengths[:len(predicted.track_index)] != _up(fallback, cuda)).any()
    assert bool(own) == bool(want_known[predicted.track_index.cpu().numpy()].any()), 'a followed person is placed with their own skeleton'
    learn.reset()
    assert learn.bones is None and learn.tracks is None
    print(f'{precision}: {int(stats[..., 2].sum())} lengths accepted, {int(stats[..., 3].sum())} '
          f'rejected, {int(read.known.sum())} of {read.known.numel()} (slot, bone) pairs known, {predicted.n_predicted} predicted boxes')


@gpu
def test_placement_with_device_bone_lengths_is_placement_with_their_host_copy(cuda, tmp_path):
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_single_view import _same
    from tests.test_gpu_world_follow import _rig
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi, _ = _rig()
    n, e = len(boxes), len(spec.skeleton.head_edges)
    host = np.random.default_rng(4).uniform(150.0, 450.0, (n, e))
    device = _up(host, cuda)
    dboxes, dfi = _up(boxes, cuda), _up(fi, cuda)
    for views in (None, 3):
        for b, f in ((boxes, fi), (dboxes, dfi)):
            kw = dict(cameras=cams, frame_index=f, precision='f16', views=views, coords='world')
            want = FR.locate_poses_in_frames(frames, b, path, bone_lengths=host, **kw)
            got = FR.locate_poses_in_frames(frames, b, path, bone_lengths=device, **kw)
            assert _same(got.poses, want.poses) and _same(got.keypoints2d, want.keypoints2d) and _same(got.z_offset, want.z_offset)
            assert torch.isfinite(got.poses).all()
    assert torch.equal(device, _up(host, cuda)), 'the tensor is read, never written'
    for bad in (device[:, :-1], device.to(torch.float32), device.t().contiguous().t(), device[:-1]):
        with pytest.raises(ValueError, match='a tensor as bone_lengths must be'):
            FR.locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, bone_lengths=bad, precision='f16')
