"""metro_warp_crops_frames_u8 and estimate_pose_in_frames on the MI355X: bytes against metro_warp_crop_u8 and the oracle,
one launch against per-frame launches, poses against the oracle forward and against estimate_pose on the same crops."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd.frames import Camera, CropParams, crop_params, warp_frames
from tests import oracle_frames as OP

pytestmark = pytest.mark.gpu


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _oracle_crops(frames, p, fi, side):
    return OP.crop_frames_u8(frames, fi, p.mode, p.homography, p.partial, p.intrinsics, p.distortion, side)


def _cameras():
    from tests.test_frames import FIX, fixture_cameras
    d = np.load(FIX)
    cams = fixture_cameras(d)
    cams[2].distortion_coeffs = np.zeros(5, np.float32)      # the intrinsics-only camera in the general mode too
    return d, cams


def test_homography_mode_matches_warp_crop_u8(cuda):
    from metro_pose3d_amd.preprocess import box_homography, warp_crops
    ang = 0.15
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    from metro_pose3d_amd.preprocess import homography_between_cameras
    homs = np.stack([box_homography((50, 20, 200, 260)), box_homography((-40, -40, 200, 200)),
                     box_homography((1700, 900, 300, 300)), np.array([[1, 0, 5000], [0, 1, 0], [0, 0, 1]], np.float32),
                     homography_between_cameras(np.array([[1100., 0, 320], [0, 1100, 240], [0, 0, 1]]), np.eye(3),
                                                np.array([[900., 0, 128], [0, 900, 128], [0, 0, 1]]), rot)])
    n = len(homs)
    padded = torch.from_numpy(_frame(300, 440, 3)).to(cuda)[:, :400]          # row stride 1320 > 3 * 400
    for frame in (torch.from_numpy(_frame(300, 400, 1)).to(cuda), torch.from_numpy(_frame(1080, 1920, 2)).to(cuda), padded):
        p = CropParams(np.zeros(n, np.int32), homs, np.zeros((n, 3, 3)), np.zeros((n, 3, 3), np.float32),
                       np.zeros((n, 5), np.float32), None, None)
        got = warp_frames([frame], p, np.zeros(n), 256)
        ref = warp_crops(frame.contiguous(), homs, 256)
        assert torch.equal(got, ref), tuple(frame.shape)
        if frame.stride(0) != 3 * frame.shape[1]:
            assert frame.stride(0) == 1320                               # warp_frames passed the stride, no copy


def test_general_mode_matches_the_oracle(cuda):
    """Three cameras (H36M-like, 3DHP, intrinsics-only with zero coefficients), boxes inside, partly outside and wholly
    outside the frame, and one crop whose rays partly point behind the camera (zeros there, no fault)."""
    d, cams = _cameras()
    frames = [_frame(*d[f'cam{i}_frame_hw'], seed=10 + i) for i in range(3)]
    boxes = np.concatenate([d['boxes'], [[-4000, 200, 300, 400], [1300, 1300, 150, 200], [-900, -900, 300, 300]]])
    fi = np.concatenate([d['box_camera'], [2, 0, 1]]).astype(np.int64)
    p = crop_params(cams, boxes, fi, 256)
    assert (p.mode == _lib.METRO_WARP_DISTORTED).all()
    ang = np.deg2rad(80)
    ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    p.partial[-1] = ry @ np.linalg.inv(np.array([[200., 0, 128], [0, 200, 128], [0, 0, 1]]))     # behind the camera for x > ~163
    got = warp_frames([torch.from_numpy(f) for f in frames], p, fi, 256, device=cuda).cpu().numpy()
    ref = _oracle_crops(frames, p, fi, 256)
    for i in range(len(fi)):
        diff = got[i] != ref[i]
        assert not diff.any(), f'crop {i}: {int(diff.sum())} values differ, max {np.abs(got[i] - ref[i]).max() * 255:.2f} LSB'
    mx, _ = OP.distorted_crop_coordinates(p.partial[-1], p.intrinsics[-1], p.distortion[-1], 256)
    assert np.isnan(mx).any() and (got[-1][np.isnan(mx)] == 0).all() and (got[-1] > 0).any()
    assert (got[:len(d['boxes'])] > 0).any(axis=(1, 2, 3)).all() and (got[-3] == 0).all()      # -3: wholly outside


def test_one_launch_equals_per_frame_launches(cuda):
    sizes = [(300, 400), (1080, 1920), (720, 1280), (64, 48), (1002, 1000), (480, 640), (257, 333), (1080, 1920)]
    frames = [torch.from_numpy(_frame(h, w, 20 + k)).to(cuda) for k, (h, w) in enumerate(sizes)]
    rng = np.random.default_rng(4)
    fi = rng.permutation(np.repeat(np.arange(8), 3))
    cams = [Camera(np.array([[w * 0.9, 0, w / 2], [0, w * 0.9, h / 2], [0, 0, 1]]),
                   None if k % 2 else np.float32([-0.2, 0.1, 0.001, -0.002, 0.01])) for k, (h, w) in enumerate(sizes)]
    boxes = np.array([[rng.uniform(-0.1, 0.8) * sizes[f][1], rng.uniform(-0.1, 0.8) * sizes[f][0],
                       rng.uniform(0.1, 0.5) * sizes[f][1], rng.uniform(0.1, 0.5) * sizes[f][0]] for f in fi])
    p = crop_params(cams, boxes, fi, 256)
    together = warp_frames(frames, p, fi, 256)
    for k in range(8):
        sel = np.flatnonzero(fi == k)
        part = CropParams(*(a[sel] for a in p))
        alone = warp_frames([frames[k]], part, np.zeros(len(sel)), 256)
        assert torch.equal(together[torch.from_numpy(sel).to(cuda)], alone), k
    with pytest.raises(ValueError, match='frame_index'):
        warp_frames(frames, p, np.full(len(fi), 8), 256)


def _model(tmp_path, dataset='h36m'):
    from metro_pose3d_amd import ModelSpec, save_model, synth
    spec = ModelSpec(50, 32, dataset, base_width=8)
    params = synth.make_params(50, spec.n_head_channels, 8, seed=1, logit_gain=0.84)
    path = str(tmp_path / f'toy_{dataset}.npz')
    save_model(path, spec, params)
    return spec, params, path


def test_estimate_pose_in_frames_f64_matches_the_oracle(cuda, tmp_path):
    from metro_pose3d_amd.frames import estimate_pose_in_frames
    from oracle import forward as OF
    from oracle import heads as OH
    from tests import helpers as H
    spec, params, path = _model(tmp_path)
    d, cams = _cameras()
    cams[2].distortion_coeffs = None
    frames = [_frame(*d[f'cam{i}_frame_hw'], seed=30 + i) for i in range(3)]
    sel = [0, 2, 8, 11, 14, 16]
    boxes, fi = d['boxes'][sel], d['box_camera'][sel]
    poses, edges, names = estimate_pose_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, precision='f64')
    assert poses.shape == (6, 17, 3) and poses.is_cuda and names[0] == b'pelv' and edges.shape == (16, 2)
    p = crop_params(cams, boxes, fi, 256)
    crops = _oracle_crops(frames, p, fi, 256)
    ref = OF.forward(H.oracle_spec(spec), params, crops, torch.float64).numpy()
    ref_cam = OH.to_orig_cam(ref, p.rot_to_orig_cam, spec.skeleton.out_mirror)
    assert np.abs(poses.cpu().numpy() - ref_cam).max() <= 1e-3
    world = estimate_pose_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, coords='world', precision='f64')[0]
    assert np.abs(world.cpu().numpy() - OH.to_orig_cam(ref, p.rot_to_world, spec.skeleton.out_mirror)).max() <= 1e-3


@pytest.mark.parametrize('dataset', ['h36m', 'many19'])
def test_estimate_pose_in_frames_f16_is_estimate_pose_on_the_crops(cuda, tmp_path, dataset):
    from metro_pose3d_amd.frames import estimate_pose_in_frames
    from metro_pose3d_amd.heads import to_orig_cam
    from metro_pose3d_amd.inference import estimate_pose
    spec, params, path = _model(tmp_path, dataset)
    d, cams = _cameras()
    frames = [torch.from_numpy(_frame(*d[f'cam{i}_frame_hw'], seed=40 + i)).to(cuda) for i in range(3)]
    boxes, fi = d['boxes'], d['box_camera']
    p = crop_params(cams, boxes, fi, 256)
    crops = warp_frames(frames, p, fi, 256)
    base = estimate_pose(crops, path, precision='f16')[0]
    got = estimate_pose_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, coords='crop', precision='f16')[0]
    assert torch.equal(got, base)
    cam = estimate_pose_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, precision='f16')[0]
    assert torch.equal(cam, to_orig_cam(base, p.rot_to_orig_cam, spec.skeleton.out_mirror))
    # no cameras: the axis-aligned crops of box_homography, the camera frame is the crop frame
    plain = estimate_pose_in_frames(frames[0], boxes[:3], path, precision='f16')[0]
    q = crop_params(None, boxes[:3], np.zeros(3), 256)
    assert torch.equal(plain, estimate_pose(warp_frames(frames[0], q, np.zeros(3), 256), path, precision='f16')[0])
    with pytest.raises(ValueError, match='coords'):
        estimate_pose_in_frames(frames, boxes, path, coords='image')
