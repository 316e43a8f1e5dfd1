"""Host camera geometry of the frame pipeline (frames.py), pure NumPy: the reference's camera restated in its dtypes.

The reference's test path (src/data/data_loading.py:33-58, 107-111) builds a virtual camera per person box that turns towards
the box centre, drops the lens distortion, squares the pixels and zooms so the box fills the crop (cameralib.look_at_box,
src/cameralib.py:337-358); under --test-aug it zooms, rolls and flips that camera per view (data_loading.py:60-68, 77).

  Camera, undistort_points, look_at_box   the reference's camera (fp32 R, K, t) and the virtual camera of a crop
  euler2mat_ryxz, view_camera             a test-time view of a look_at_box camera
  _square_crop_camera                     the square crop of a call without cameras, as a camera

Divergence from the reference, on purpose:
  * a Camera built from intrinsics alone (no R, no t) defaults to world_up = (0, -1, 0), not the reference's (0, 0, 1): with
    R = I and t = 0, `turn_towards` takes cross(new_z, (0, 0, 1)), which vanishes for a box near the optical axis.
"""
from __future__ import annotations

import copy
import math
from typing import Sequence

import numpy as np

UNDISTORT_ITERATIONS = 5


def undistort_points(points, intrinsic_matrix, distortion_coeffs) -> np.ndarray:
    """cv2.undistortPoints(points, K, D) with R = P = None -> float32 [N, 2] normalised camera coordinates.

    OpenCV is absent here, so this is restated from its published source, modules/imgproc/src/undistort.cpp
    (cvUndistortPoints / cvUndistortPointsInternal, 3.x): K and D converted to double; fx, fy, cx, cy only (a skew term is
    ignored); x = (u - cx) * (1 / fx); with coefficients, the fixed-point iteration
        icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2),  x = (x0 - dx) icdist
    run for the fixed count of the default criteria, TermCriteria(COUNT, 5, 0.01) (`iters = 5` in the older 3.x form), then
    the result is stored as float32 like the float32 input.  PARITY UNPINNED against cv2 itself (no OpenCV to execute)."""
    p = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    a = np.asarray(intrinsic_matrix, np.float64)
    fx, fy, cx, cy = a[0, 0], a[1, 1], a[0, 2], a[1, 2]
    ifx, ify = 1. / fx, 1. / fy
    x = (p[:, 0] - cx) * ifx
    y = (p[:, 1] - cy) * ify
    if distortion_coeffs is not None:
        k = np.zeros(14)
        d = np.asarray(distortion_coeffs, np.float64).ravel()
        k[:len(d)] = d
        x0, y0 = x, y
        for _ in range(UNDISTORT_ITERATIONS):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            delta_x = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            delta_y = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - delta_x) * icdist
            y = (y0 - delta_y) * icdist
    return np.stack([x, y], axis=-1).astype(np.float32)


class Camera:
    """The parts of the reference's cameralib.Camera (src/cameralib.py:25-84) the frame pipeline needs, in its dtypes:
    R (world -> camera rotation), t (optical centre in world coordinates) and the intrinsic matrix are float32, the
    distortion coefficients (k1, k2, p1, p2, k3; OpenCV order) float32 or None.

    world_up defaults to (0, 0, 1) like the reference when R or t is given; a camera built from intrinsics alone defaults to
    (0, -1, 0) (image y points down, so "up" is -y): the reference default degenerates there (module docstring)."""

    def __init__(self, intrinsic_matrix, distortion_coeffs=None, R=None, t=None, world_up=None):
        if world_up is None:
            world_up = (0, -1, 0) if R is None and t is None else (0, 0, 1)
        self.R = np.asarray(np.eye(3) if R is None else R, np.float32)
        self.t = np.asarray(np.zeros(3) if t is None else t, np.float32)
        self.intrinsic_matrix = np.asarray(intrinsic_matrix, np.float32)
        self.distortion_coeffs = None if distortion_coeffs is None else np.asarray(distortion_coeffs, np.float32)
        self.world_up = np.asarray(world_up)
        if self.R.shape != (3, 3) or self.t.shape != (3,) or self.intrinsic_matrix.shape != (3, 3):
            raise ValueError('R and intrinsic_matrix must be 3x3, t a 3-vector')
        if not np.allclose(self.intrinsic_matrix[2, :], [0, 0, 1]):
            raise ValueError(f'bottom row of the intrinsic matrix must be (0, 0, 1), got {self.intrinsic_matrix[2, :]}')
        if self.distortion_coeffs is not None and self.distortion_coeffs.shape != (5,):
            raise ValueError(f'distortion_coeffs must be None or 5 values (k1, k2, p1, p2, k3), got '
                             f'{self.distortion_coeffs.shape}')

    def copy(self) -> 'Camera':
        return copy.deepcopy(self)

    # cameralib.py:133-156
    def world_to_camera(self, points):
        return (np.asarray(points, np.float32) - self.t) @ self.R.T

    def camera_to_world(self, points):
        return np.asarray(points, np.float32) @ np.linalg.inv(self.R).T + self.t

    def camera_to_image_undistorted(self, points):
        """camera_to_image (:126-131) of a camera without distortion coefficients."""
        assert self.distortion_coeffs is None
        projected = points[:, :2] / points[:, 2:]
        return projected @ self.intrinsic_matrix[:2, :2].T + self.intrinsic_matrix[:2, 2]

    def image_to_camera(self, points):
        p = undistort_points(points, self.intrinsic_matrix, self.distortion_coeffs)
        return np.concatenate([p, np.ones_like(p[:, :1])], axis=1)        # convertPointsToHomogeneous, depth 1

    def image_to_world(self, points):
        return self.camera_to_world(self.image_to_camera(points))

    # cameralib.py:167-228
    def turn_towards(self, target_image_point):
        target_world_point = self.image_to_world(np.asarray([target_image_point], np.float64))[0]
        new_z = target_world_point - self.t
        new_z = new_z / np.linalg.norm(new_z)
        new_x = np.cross(new_z, self.world_up)
        new_x = new_x / np.linalg.norm(new_x)
        new_y = np.cross(new_z, new_x)
        self.R = np.vstack([new_x, new_y, new_z]).astype(np.float32)

    def undistort(self):
        self.distortion_coeffs = None

    def square_pixels(self):
        fx, fy = self.intrinsic_matrix[0, 0], self.intrinsic_matrix[1, 1]
        fmean = 0.5 * (fx + fy)
        multiplier = np.array([[fmean / fx, 0, 0], [0, fmean / fy, 0], [0, 0, 1]])     # float64, so K becomes float64
        self.intrinsic_matrix = multiplier @ self.intrinsic_matrix

    def zoom(self, factor):
        self.intrinsic_matrix[:2, :2] *= np.expand_dims(factor, -1)

    def center_principal_point(self, imshape):
        self.intrinsic_matrix[:2, 2] = [imshape[1] / 2, imshape[0] / 2]

    # cameralib.py:95-98, 191-192
    def rotate(self, yaw=0, pitch=0, roll=0):
        """R <- euler2mat(yaw, pitch, roll, 'ryxz')^T R (angles in radians): the camera turns by yaw about its y axis, then
        pitch about its new x axis, then roll about its new optical axis.  R becomes float64, as in the reference."""
        self.R = euler2mat_ryxz(yaw, pitch, roll).T @ self.R

    def horizontal_flip(self):
        self.R[0] *= -1


def euler2mat_ryxz(yaw, pitch, roll) -> np.ndarray:
    """transforms3d.euler.euler2mat(yaw, pitch, roll, 'ryxz') (transforms3d is not a dependency), float64 [3, 3].

    'ryxz' is the rotating-frame convention with axes y, x, z: the matrix is Ry(yaw) @ Rx(pitch) @ Rz(roll) with the
    right-handed elementary rotations Rx(a) = [[1, 0, 0], [0, c, -s], [0, s, c]], Ry(a) = [[c, 0, s], [0, 1, 0], [-s, 0, c]],
    Rz(a) = [[c, -s, 0], [s, c, 0], [0, 0, 1]].  Its entries are written as transforms3d's euler2mat writes them for this axis
    code (first axis z, no parity, no repetition, rotating frame: i, j, k = 2, 0, 1 with the first and last angle swapped),
    so roll alone gives exactly cos(roll) and sin(roll)."""
    si, sj, sk = math.sin(roll), math.sin(pitch), math.sin(yaw)
    ci, cj, ck = math.cos(roll), math.cos(pitch), math.cos(yaw)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    m = np.eye(3)
    m[2, 2] = cj * ck
    m[2, 0] = sj * sc - cs
    m[2, 1] = sj * cc + ss
    m[0, 2] = cj * sk
    m[0, 0] = sj * ss + cc
    m[0, 1] = sj * cs - sc
    m[1, 2] = -sj
    m[1, 0] = cj * si
    m[1, 1] = cj * ci
    return m


def look_at_box(camera: Camera, box: Sequence[float], side: int = 256) -> Camera:
    """The virtual camera of a crop: reference cameralib.look_at_box (src/cameralib.py:337-358), step by step -- turn towards
    the box centre, undistort, square the pixels, zoom so that the box's longer side (measured between the two side midpoints,
    through the world) spans `side` pixels, centre the principal point.  This is the reference's stand-alone helper; the
    training loader's variant (data_loading.py:33-58: the norm of the side-point difference, a 1.05 box expansion for 3DHP,
    augmentation flags) is not what is restated here."""
    cam = camera.copy()
    box = np.asarray(box, np.float64)
    center_point = box[:2] + box[2:] / 2
    delta_x = np.array([box[2] / 2, 0])
    delta_y = np.array([0, box[3] / 2])
    if box[2] < box[3]:
        sidepoints = np.stack([center_point - delta_y, center_point + delta_y])
    else:
        sidepoints = np.stack([center_point - delta_x, center_point + delta_x])
    world_sidepoints = camera.image_to_world(sidepoints)
    cam.turn_towards(center_point)
    cam.undistort()
    cam.square_pixels()
    cam_sidepoints = cam.camera_to_image_undistorted(cam.world_to_camera(world_sidepoints))
    if box[2] < box[3]:
        crop_side = np.abs(cam_sidepoints[0, 1] - cam_sidepoints[1, 1])
    else:
        crop_side = np.abs(cam_sidepoints[0, 0] - cam_sidepoints[1, 0])
    cam.zoom(side / crop_side)
    cam.center_principal_point((side, side))
    return cam


def _roll_rad(roll_deg: float) -> float:
    return float(roll_deg) * math.pi / 180


def view_camera(camera: Camera, roll_deg: float, zoom: float, flip: bool) -> Camera:
    """A view of a look_at_box camera, as the reference's loader builds it under --test-aug (data_loading.py:60-68, 77):
    cam.zoom(zoom), cam.rotate(roll=roll), then cam.horizontal_flip() when flip."""
    cam = camera.copy()
    cam.zoom(zoom)
    cam.rotate(roll=_roll_rad(roll_deg))
    if flip:
        cam.horizontal_flip()
    return cam


def _square_crop_camera(side: int) -> Camera:
    """cameras=None: the square crop as a camera of principal point (side/2, side/2), unit focal length (roll, zoom and flip
    are image-plane similarities about that point whatever the focal length), R = I, K in float64 like look_at_box's."""
    cam = Camera(np.eye(3))
    cam.intrinsic_matrix = np.array([[1., 0, side / 2], [0, 1., side / 2], [0, 0, 1]])
    return cam
