"""CPU restatement of the camera path with lens distortion (reference src/cameralib.py:265-358).  TEST INFRASTRUCTURE:
the oracle of metro_pose3d_amd/frames.py and of metro_warp_crops_frames_u8, built on oracle/preprocess.py's restated
cv2.remap.  The product never imports it."""
from __future__ import annotations

import numpy as np

from oracle.preprocess import crop_coordinates, cv_round_x86, remap_u8_linear_constant0, reproject_image_fast  # noqa: F401

# ---- the camera path with lens distortion (reference cameralib.py:265-358) ------------------------------------------------
# `undistort_points` restates cv2.undistortPoints (OpenCV 3.x modules/imgproc/src/undistort.cpp, cvUndistortPoints, R = P =
# None): double arithmetic on fx, fy, cx, cy, x = (u - cx) * (1 / fx), five iterations of the default criteria
# TermCriteria(COUNT, 5, 0.01) when coefficients are given, float32 result.  PARITY UNPINNED against cv2 itself.

def undistort_points(points, k, dist):
    p = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    k = np.asarray(k, np.float64)
    u = (p[:, 0] - k[0, 2]) * (1. / k[0, 0])
    v = (p[:, 1] - k[1, 2]) * (1. / k[1, 1])
    if dist is not None:
        k1, k2, p1, p2, k3 = (float(c) for c in np.asarray(dist, np.float64).ravel())
        u0, v0 = u, v
        for _ in range(5):
            r2 = u * u + v * v
            icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            du = 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
            dv = p1 * (r2 + 2 * v * v) + 2 * p2 * u * v
            u, v = (u0 - du) * icdist, (v0 - dv) * icdist
    return np.stack([u, v], -1).astype(np.float32)


def project_points(points, k, dist):
    """cameralib.project_points (:375-397) on float32 [N, 3] camera points, in its statement order (float32 throughout);
    the final [N, 2] @ K[:2, :2].T is evaluated fma(y, K01, rn(x K00)) like the BLAS order of crop_coordinates."""
    f32 = np.float32
    k = np.asarray(k, f32)
    d = np.asarray(dist, f32)
    pts = np.asarray(points, f32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        px, py = pts[:, 0] / pts[:, 2], pts[:, 1] / pts[:, 2]
        r2 = px * px + py * py
        r4 = r2 * r2
        dd = d[0] * r2
        dd = dd + d[1] * r4
        r6 = r4 * r2
        dd = dd + d[4] * r6
        dd = dd + f32(1)
        dd = dd + px * (f32(2) * d[3])
        dd = dd + py * (f32(2) * d[2])
        px = px * dd + r2 * d[3]
        py = py * dd + r2 * d[2]
        fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)
        u = fma(py, k[0, 1], px * k[0, 0]) + k[0, 2]
        v = fma(py, k[1, 1], px * k[1, 0]) + k[1, 2]
    return u, v


def distorted_crop_coordinates(partial, k, dist, side: int):
    """mapx, mapy float32 [side, side] of reproject_image case 2 (cameralib.py:297-312) for an original camera with
    distortion: ray = partial (x, y, 1) in float64 as rn(rn(rn(P0 x) + rn(P1 y)) + P2) (the fp32 grid promoted against the
    float64 partial_homography; NumPy's matmul may sum in another order: within an ulp), cast to float32 as project_points'
    entry does, then project_points.  A ray with z <= 0 gives NaN (the border value 0), where the reference would project
    it through the origin."""
    pmat = np.asarray(partial, np.float64)
    y, x = np.mgrid[:side, :side].astype(np.float32)
    x, y = x.ravel().astype(np.float64), y.ravel().astype(np.float64)
    ray = np.stack([((pmat[r, 0] * x) + (pmat[r, 1] * y)) + pmat[r, 2] for r in range(3)], -1).astype(np.float32)
    u, v = project_points(ray, k, dist)
    behind = ~(ray[:, 2] > 0)
    u[behind] = np.nan
    v[behind] = np.nan
    return u.reshape(side, side), v.reshape(side, side)


def look_at_box(k, dist, rot, t, world_up, box, side: int):
    """cameralib.look_at_box (:337-358) -> (virtual K float64, virtual R float32), in the reference's dtypes: the fp32 camera,
    cross products against the (integer) world_up in float64, square_pixels' float64 multiplier."""
    k = np.asarray(k, np.float32)
    rot = np.asarray(rot, np.float32)
    t = np.asarray(t, np.float32)
    box = np.asarray(box, np.float64)
    center = box[:2] + box[2:] / 2
    axis = 1 if box[2] < box[3] else 0
    delta = np.zeros(2)
    delta[axis] = box[2 + axis] / 2
    sides = np.stack([center - delta, center + delta])

    def image_to_world(pts):
        cam = undistort_points(pts, k, dist)
        cam = np.concatenate([cam, np.ones_like(cam[:, :1])], 1)
        return cam @ np.linalg.inv(rot).T + t

    world_sides = image_to_world(sides)
    z = image_to_world(center[None])[0] - t
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.asarray(world_up))
    x = x / np.linalg.norm(x)
    r_new = np.stack([x, np.cross(z, x), z]).astype(np.float32)
    fx, fy = k[0, 0], k[1, 1]
    fmean = 0.5 * (fx + fy)
    k_new = np.array([[fmean / fx, 0, 0], [0, fmean / fy, 0], [0, 0, 1]]) @ k
    cam_sides = (world_sides - t) @ r_new.T
    im_sides = (cam_sides[:, :2] / cam_sides[:, 2:]) @ k_new[:2, :2].T + k_new[:2, 2]
    k_new[:2, :2] *= side / np.abs(im_sides[0, axis] - im_sides[1, axis])
    k_new[:2, 2] = [side / 2, side / 2]
    return k_new, r_new


def crop_frames_u8(frames, frame_index, mode, homography, partial, intrinsics, distortion, side: int) -> np.ndarray:
    """-> float32 [n, side, side, 3] in [0, 1]: crop i of frames[frame_index[i]] through its homography (mode 0,
    reproject_image_fast) or its distorted camera (mode 1, reproject_image case 2), remap_u8_linear_constant0, /255."""
    out = []
    for i, f in enumerate(frame_index):
        if mode[i] == 0:
            mapx, mapy = crop_coordinates(homography[i], side)
        else:
            mapx, mapy = distorted_crop_coordinates(partial[i], intrinsics[i], distortion[i], side)
        im = remap_u8_linear_constant0(np.asarray(frames[f]), mapx, mapy).astype(np.float32) / np.float32(255)
        out.append(np.minimum(np.maximum(np.float32(-1), im), np.float32(1)))
    return np.stack(out) if out else np.zeros((0, side, side, 3), np.float32)
