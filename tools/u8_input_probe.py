#!/usr/bin/env python3
"""uint8 crops against float32 crops: what the byte path buys, layer by layer and end to end.

    python tools/u8_input_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights), f16, at 64 and 256 crops.  Every comparison runs its arms INTERLEAVED, window by
window, in one process: A (float32), B (uint8), A again.  The two float32 arms are the same code on the same data: their
relative difference (`aa_spread`) is the noise margin a uint8-vs-float32 difference has to beat.
  * stem launch: metro_stem_pool_f32in against metro_stem_pool_u8in (the C entries alone), device events around 100
    back-to-back launches after 20 warm-up launches, median of 5 windows; VGPRs and LDS from the compiler's resource report;
  * warp launch: metro_warp_crops_frames_u8 against metro_warp_crops_frames_u8_to_u8, 64 / 256 boxes from 8 device frames of
    1920 x 1080, homography and distorted mode, timed the same way;
  * Engine.forward crops/s from device-resident float32 and uint8 crops;
  * estimate_pose crops/s from host float32 and host uint8 crops (pageable torch tensors, as a user passes them);
  * estimate_pose_in_frames crops/s for both crop_dtypes, 64 boxes as a CUDA tensor (device geometry), from 8 device frames
    and from 8 host frames;
host clock around calls that end in a synchronisation, after 3 warm-up calls, median of 5 windows.
For the kernel rows of the profiler: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/u8_input_probe.py --quick
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, _lib, save_model, synth  # noqa: E402
from metro_pose3d_amd import frames as FR  # noqa: E402
from metro_pose3d_amd.engine import Engine  # noqa: E402
from metro_pose3d_amd.frames import Camera, crop_params, estimate_pose_in_frames  # noqa: E402
from metro_pose3d_amd.inference import estimate_pose  # noqa: E402

# hipcc -Rpass-analysis=kernel-resource-usage on csrc/stem_pool_f16.hip (gfx950): both kernels 2 waves per SIMD, no spills
STEM_RESOURCES = {'float32': {'kernel': 'stem_pool_rows_kernel', 'vgprs': 240, 'lds_bytes': 81536},
                  'uint8': {'kernel': 'stem_pool_rows_u8_kernel', 'vgprs': 241, 'lds_bytes': 56960}}


def _summary(res, higher_is_better):
    med = {k: statistics.median(v) for k, v in res.items()}
    out = {k: {'median': round(med[k], 2), 'windows': [round(x, 2) for x in v]} for k, v in res.items()}
    a = 0.5 * (med['float32'] + med['float32_again'])
    out['aa_spread'] = round(abs(med['float32'] - med['float32_again']) / a, 4)
    gain = med['uint8'] / a if higher_is_better else a / med['uint8']
    out['uint8_over_float32'] = round(gain, 4)            # > 1: uint8 is faster
    return out


def ab_launch_us(f32, u8, windows, iters):
    """us per launch, the three arms interleaved window by window."""
    arms = (('float32', f32), ('uint8', u8), ('float32_again', f32))
    for _, fn in arms:
        for _ in range(20):
            fn()
    res = {k: [] for k, _ in arms}
    for _ in range(windows):
        for k, fn in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / iters)
    return _summary(res, higher_is_better=False)


def ab_per_s(f32, u8, units, windows, calls, sync):
    """units per second, the three arms interleaved window by window; every window ends in a synchronisation."""
    arms = (('float32', f32), ('uint8', u8), ('float32_again', f32))
    for _, fn in arms:
        for _ in range(3):
            fn()
    sync()
    res = {k: [] for k, _ in arms}
    for _ in range(windows):
        for k, fn in arms:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            res[k].append(units * calls / (time.perf_counter() - t0))
    return _summary(res, higher_is_better=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('u8_input_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 10, 1) if opts.quick else (5, 100, 4)
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    rng = np.random.default_rng(0)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    spec = ModelSpec(50, 16, 'h36m')
    side = spec.proc_side
    result = {'device': torch.cuda.get_device_name(dev),
              'what': 'RN50 stride 16 h36m (synthetic weights), f16; arms interleaved window by window: float32, uint8, '
                      'float32 again; aa_spread = |float32 - float32_again| / their mean; uint8_over_float32 > 1: uint8 faster',
              'stem_resources': STEM_RESOURCES}
    host_frames = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]
    frames = [torch.from_numpy(f).to(dev) for f in host_frames]
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    dist = np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309])
    cameras = {'homography': Camera(k), 'distorted': Camera(k, dist)}
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    wp = np.zeros((64, 7, 8, 4), np.float16)
    wp[:, :, :7, :3] = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float16)
    tw, tb = torch.from_numpy(wp).to(dev), torch.from_numpy(rng.standard_normal(64).astype(np.float32)).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        for n in (64, 256):
            h8 = torch.from_numpy(rng.integers(0, 256, (n, side, side, 3), dtype=np.uint8))       # pageable host tensors
            h32 = h8.to(torch.float32) / 255
            d8, d32 = h8.to(dev), h32.to(dev)
            # stem launch
            out = torch.empty((n, side // 4, side // 4, 64), dtype=torch.float16, device=dev)
            f32 = lambda: _lib.check(lib.metro_stem_pool_f32in(p(d32), p(tw), p(tb), p(out), n, side, stream), 'stem f32in')
            u8 = lambda: _lib.check(lib.metro_stem_pool_u8in(p(d8), p(tw), p(tb), p(out), n, side, stream), 'stem u8in')
            result[f'stem_launch_us_{n}'] = ab_launch_us(f32, u8, windows, iters)
            # warp launch
            fi = np.repeat(np.arange(8), n // 8)
            boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
            c32 = torch.empty((n, side, side, 3), dtype=torch.float32, device=dev)
            c8 = torch.empty((n, side, side, 3), dtype=torch.uint8, device=dev)
            for mode, cam in cameras.items():
                recs = FR._upload(FR.pack_crops(crop_params(cam, boxes, fi, side), fi), dev)
                f32 = lambda: FR._launch_warp(frames, recs, n, side, c32, dev)
                u8 = lambda: FR._launch_warp(frames, recs, n, side, c8, dev)
                result[f'warp_launch_us_{n}_{mode}'] = ab_launch_us(f32, u8, windows, iters)
            # Engine.forward from device-resident crops
            eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
            poses = torch.empty((n, spec.skeleton.n_out, 3), dtype=torch.float32, device=dev)
            result[f'forward_crops_per_s_device_{n}'] = ab_per_s(lambda: eng.forward(d32, out=poses), lambda: eng.forward(d8, out=poses),
                                                                 n, windows, 4 * calls, sync)
            eng.close()
            # estimate_pose from host crops
            result[f'estimate_pose_crops_per_s_host_{n}'] = ab_per_s(lambda: estimate_pose(h32, path, precision='f16'),
                                                                     lambda: estimate_pose(h8, path, precision='f16'),
                                                                     n, windows, calls, sync)
        # the frames chain: 64 boxes, device geometry
        fi = np.repeat(np.arange(8), 8)
        boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
        d_boxes, d_fi = torch.from_numpy(boxes).to(dev), torch.from_numpy(fi).to(dev)
        for where, fr in (('device_frames', frames), ('host_frames', host_frames)):
            for mode, cam in cameras.items():
                call = lambda dt: estimate_pose_in_frames(fr, d_boxes, path, cameras=cam, frame_index=d_fi, precision='f16', crop_dtype=dt)
                result[f'estimate_pose_in_frames_crops_per_s_{where}_{mode}'] = ab_per_s(lambda: call('float32'), lambda: call('uint8'),
                                                                                          64, windows, calls, sync)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
