"""metro_warp_crops_frames_planes on the MI355X: NV12, I420 and BGR frames against metro_warp_crops_frames_u8 on the RGB frame
that tests/oracle_yuv.py converts them to (torch.equal), from every frame layout and from host frames, mixed formats in one
launch, and the pose calls from NV12 frames against the same calls on RGB frames (bit-equal)."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd import frames as FR
from metro_pose3d_amd.frames import Camera, CropParams, crop_params, estimate_pose_in_frames, locate_poses_in_frames, warp_frames
from tests import oracle_yuv as OY

pytestmark = pytest.mark.gpu

SIZES = [(1080, 1920), (48, 64)]
CASES = [('nv12', 'bt601'), ('nv12', 'bt709'), ('i420', 'bt601'), ('i420', 'bt709'), ('bgr', 'bt601')]


def _frames(fmt, matrix, seed0=0):
    """-> (one-array frames in fmt, the RGB frames they stand for), host uint8."""
    src, rgb = [], []
    for k, (h, w) in enumerate(SIZES):
        y, u, v = OY.random_planes(h, w, seed0 + k)
        if fmt == 'bgr':
            rgb.append(OY.yuv420_to_rgb(y, u, v))
            src.append(np.ascontiguousarray(rgb[-1][..., ::-1]))
        else:
            src.append(OY.nv12_frame(y, u, v) if fmt == 'nv12' else OY.i420_frame(y, u, v))
            rgb.append(OY.to_rgb(src[-1], fmt, matrix))
    return src, rgb


def _params(distorted):
    """Crops of both frames: boxes inside, partly outside and wholly outside; in the distorted mode one crop whose rays
    partly point behind the camera."""
    boxes, fi = [], []
    for k, (h, w) in enumerate(SIZES):
        boxes += [[0.2 * w, 0.1 * h, 0.3 * w, 0.6 * h], [-0.2 * w, 0.5 * h, 0.5 * w, 0.8 * h], [3 * w, 3 * h, 0.2 * w, 0.2 * h],
                  [0.6 * w, -0.1 * h, 0.25 * w, 0.3 * h]]
        fi += [k] * 4
    boxes, fi = np.array(boxes), np.array(fi)
    if not distorted:
        return crop_params(None, boxes, fi, 256), fi
    cams = [Camera(np.array([[w * 0.8, 0, w / 2], [0, w * 0.8, h / 2], [0, 0, 1]]), np.float32([-0.25, 0.1, 0.002, -0.001, 0.01]))
            for h, w in SIZES]
    p = crop_params(cams, boxes, fi, 256)
    assert (p.mode == _lib.METRO_WARP_DISTORTED).all()
    ang = np.deg2rad(60)                    # crop 3 (frame 0): rays with x > ~243 point behind the camera
    ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    p.partial[3] = ry @ np.linalg.inv(np.array([[200., 0, 128], [0, 200, 128], [0, 0, 1]]))
    return p, fi


@pytest.mark.parametrize('distorted', [False, True])
@pytest.mark.parametrize('fmt,matrix', CASES)
def test_crops_are_the_rgb_warp_of_the_converted_frame(cuda, fmt, matrix, distorted):
    src, rgb = _frames(fmt, matrix)
    p, fi = _params(distorted)
    dev = [torch.from_numpy(f).to(cuda) for f in src]
    got = warp_frames(dev, p, fi, 256, pixel_format=fmt, color_matrix=matrix)
    want = warp_frames([torch.from_numpy(f).to(cuda) for f in rgb], p, fi, 256)
    assert torch.equal(got, want), (fmt, matrix, distorted, int((got != want).sum()))
    g = got.cpu().numpy()
    assert (g[[0, 4]] > 0).any(axis=(1, 2, 3)).all()
    if distorted:
        assert (g[3, :, 250:] == 0).all() and (g[3] > 0).any()                    # rays behind the camera: zeros
    else:
        assert (g[[2, 6]] == 0).all()                                             # wholly outside: black


def test_every_layout_and_host_frames_give_the_same_bytes(cuda):
    (h, w), pitch = SIZES[0], 2048
    y, u, v = OY.random_planes(h, w, 5)
    rgb = OY.yuv420_to_rgb(y, u, v, 'bt709')
    p, fi = _params(True)
    sel = fi == 0
    p = CropParams(*(a[sel] for a in p))
    fi = fi[sel]
    want = warp_frames(torch.from_numpy(rgb).to(cuda), p, fi, 256)
    uv = np.stack([u, v], -1)
    # one pitched allocation, as a decoder surface: Y rows at 2048 bytes, the UV plane from an aligned offset
    surf = torch.zeros(h * pitch + 4096 + (h // 2) * pitch, dtype=torch.uint8, device=cuda)
    ys = surf[:h * pitch].view(h, pitch)[:, :w]
    uvs = surf[h * pitch + 4096:].view(h // 2, pitch)[:, :w]
    ys.copy_(torch.from_numpy(y))
    uvs.copy_(torch.from_numpy(uv.reshape(h // 2, w)))
    pitched = torch.zeros((h * 3 // 2, pitch), dtype=torch.uint8, device=cuda)
    pitched[:, :w] = torch.from_numpy(OY.nv12_frame(y, u, v))
    i420_dev = (torch.from_numpy(y).to(cuda), torch.from_numpy(u).to(cuda), torch.from_numpy(v).to(cuda))
    i420_pitched = [torch.zeros((n, pitch), dtype=torch.uint8, device=cuda) for n in (h, h // 2, h // 2)]
    for t, a in zip(i420_pitched, (y, u, v)):
        t[:, :a.shape[1]] = torch.from_numpy(a)
    i420_pitched = (i420_pitched[0][:, :w], i420_pitched[1][:, :w // 2], i420_pitched[2][:, :w // 2])
    layouts = [
        ('nv12', (ys, uvs)), ('nv12', (ys, uvs.view(h // 2, w // 2, 2))), ('nv12', pitched[:, :w]),
        ('nv12', (torch.from_numpy(y).to(cuda), torch.from_numpy(uv).to(cuda))),
        ('nv12', OY.nv12_frame(y, u, v)), ('nv12', (y, uv)), ('nv12', torch.from_numpy(OY.nv12_frame(y, u, v))),
        ('i420', i420_dev), ('i420', i420_pitched), ('i420', torch.from_numpy(OY.i420_frame(y, u, v)).to(cuda)),
        ('i420', OY.i420_frame(y, u, v)), ('i420', (y, u, v)),
    ]
    for k, (fmt, frame) in enumerate(layouts):
        got = warp_frames(frame, p, fi, 256, pixel_format=fmt, color_matrix='bt709', device=cuda)
        assert torch.equal(got, want), (k, fmt)
    assert ys.stride(0) == pitch                                   # passed with its pitch, not copied
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    for frame in (bgr, torch.from_numpy(bgr).to(cuda), torch.from_numpy(np.ascontiguousarray(bgr.transpose(1, 0, 2))).to(cuda)
                  .transpose(0, 1)):
        assert torch.equal(warp_frames(frame, p, fi, 256, pixel_format='bgr', device=cuda), want)


def test_one_launch_of_mixed_formats_equals_per_format_launches(cuda):
    parts = []
    for k, (fmt, matrix) in enumerate(CASES + [('rgb', 'bt601')]):
        src, rgb = _frames('nv12' if fmt == 'rgb' else fmt, matrix, seed0=10 * k)
        if fmt == 'rgb':
            src = rgb
        parts.append((fmt, matrix, [torch.from_numpy(f).to(cuda) for f in src]))
    p, fi = _params(True)
    n_per = len(fi)
    dev = []
    for fmt, matrix, frames in parts:
        dev += FR._device_frames(FR._frame_set(frames, 'bgr' if fmt == 'rgb' else fmt, matrix), cuda)
    for k in range(len(CASES), len(parts)):          # 'rgb' frames as METRO_PIX_RGB descriptors of the new entry
        dev[2 * k:2 * k + 2] = [d._replace(format=_lib.METRO_PIX_RGB) for d in dev[2 * k:2 * k + 2]]
    all_p = CropParams(*(np.concatenate([a] * len(parts)) for a in p))
    all_fi = np.concatenate([fi + 2 * k for k in range(len(parts))])
    out = torch.empty((len(all_fi), 256, 256, 3), dtype=torch.float32, device=cuda)
    FR._launch_warp(dev, FR._upload(FR.pack_crops(all_p, all_fi), cuda), len(all_fi), 256, out, cuda)
    for k, (fmt, matrix, frames) in enumerate(parts):
        alone = warp_frames(frames, p, fi, 256, pixel_format=fmt, color_matrix=matrix)
        assert torch.equal(out[k * n_per:(k + 1) * n_per], alone), (fmt, matrix)


def _yuv_scene(cuda):
    """The three-camera scene of the view tests with NV12 device frames, and the RGB frames they stand for."""
    from tests.test_gpu_views import _scene
    cams, rgb_frames, boxes, fi = _scene(undistorted_last=True)
    nv12, rgb = [], []
    for k, f in enumerate(rgb_frames):
        y, u, v = OY.random_planes(f.shape[0], f.shape[1], 90 + k)
        nv12.append(torch.from_numpy(OY.nv12_frame(y, u, v)).to(cuda))
        rgb.append(torch.from_numpy(OY.yuv420_to_rgb(y, u, v)).to(cuda))
    return cams, nv12, rgb, boxes, fi


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_pose_calls_from_nv12_frames_are_the_rgb_calls(cuda, tmp_path, precision):
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_views import _np
    spec, _, path = _toy_engine_model(tmp_path)
    cams, nv12, rgb, boxes, fi = _yuv_scene(cuda)
    bones = np.random.default_rng(8).uniform(200, 450, len(spec.skeleton.head_edges))
    dboxes, dfi = torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda)
    for views in (None, 5):
        for b, f in ((boxes, fi), (dboxes, dfi)):
            kw = dict(cameras=cams, frame_index=f, precision=precision, views=views)
            want = estimate_pose_in_frames(rgb, b, path, **kw)[0]
            got = estimate_pose_in_frames(nv12, b, path, pixel_format='nv12', **kw)[0]
            assert torch.equal(got, want), (views, b is dboxes)
            lw = locate_poses_in_frames(rgb, b, path, bone_lengths=bones, **kw)
            lg = locate_poses_in_frames(nv12, b, path, bone_lengths=bones, pixel_format='nv12', **kw)
            assert torch.equal(lg.poses, lw.poses) and torch.equal(lg.z_offset, lw.z_offset), (views, b is dboxes)
            assert np.array_equal(_np(lg.keypoints2d), _np(lw.keypoints2d), equal_nan=True)
    # no cameras: the axis-aligned crops of box_homography
    want = estimate_pose_in_frames(rgb, boxes, path, frame_index=fi, precision=precision)[0]
    assert torch.equal(estimate_pose_in_frames(nv12, boxes, path, frame_index=fi, precision=precision,
                                               pixel_format='nv12')[0], want)
