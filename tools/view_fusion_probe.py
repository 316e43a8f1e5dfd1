#!/usr/bin/env python3
"""What asking for the view fusion costs beside the triangulation, and that not asking costs nothing.

    python tools/view_fusion_probe.py [--out FILE] [--quick] [--grids 8,16]    # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights, J = 17), f16, 16 persons x 4 cameras = 64 crops in one forward.  Three arms
INTERLEAVED window by window in one process: triangulate (Engine.forward with coords01 and the moments, then
heads.triangulate_joints), fuse (Engine.forward_view_fusion with the internal centres: the head also stores its fp32 logits,
the three marginal launches, the triangulation launch, view_fusion, the output tensors allocated per call), triangulate again.
The two triangulate arms are the same code on the same data: their relative difference (`aa_spread`) is the noise margin the
fuse arm has to be read against.  Calls/s from a host clock around `iters` calls that end in a synchronisation, after 3 warm-up
windows, median of 5 windows, at every grid of --grids.  Nothing gates on these figures.
Per-launch times of the new kernel come from the profiler, in a run of its own per grid:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/view_fusion_probe.py --quick --grids 16
and `--stats-csv 16=<dir>/.../*_kernel_stats.csv` (repeatable) folds that table's view_fusion / triangulate / heat rows into
the JSON under `kernels`.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, heads as MH, synth  # noqa: E402
from metro_pose3d_amd.engine import Engine  # noqa: E402

PERSONS, CAMERAS = 16, 4


def rig_inputs(spec, dev):
    """PERSONS persons seen by CAMERAS ring cameras each: the records, the CSR and the mirror table on the device."""
    from tests import view_fusion_ref as VF
    case = VF.make_case(VF.head_of(spec.proc_side, spec.stride, spec.centered_stride), spec.skeleton.n_out, (CAMERAS,) * PERSONS, seed=3,
                        stride=spec.stride, spare_rows=0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(places=up(np.ascontiguousarray(case['records']).view(np.uint8).reshape(case['n'], -1)), rows=up(case['rows']),
                starts=up(case['starts']), mirror=up(np.asarray(spec.skeleton.out_mirror, np.int32)))


def calls_per_s(eng, x, rig, bufs, fusion, windows, iters):
    spec = eng.spec
    tri = lambda: (eng.forward(x, **bufs), MH.triangulate_joints(bufs['coords01'], bufs['cov01'], rig['places'].reshape(-1), rig['rows'],
                                                                 rig['starts'], spec, 'covariance'))
    fuse = lambda: eng.forward_view_fusion(x, rig['places'], rig['rows'], rig['starts'], PERSONS, rig['mirror'], fusion, 'covariance', **bufs)
    arms = (('triangulate', tri), ('fuse', fuse), ('triangulate_again', tri))
    res = {k: [] for k, _ in arms}
    for w in range(3 + windows):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            if w >= 3:
                res[name].append(iters / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in res.items()}
    a = 0.5 * (med['triangulate'] + med['triangulate_again'])
    out = {k: {'median_calls_per_s': round(med[k], 1), 'windows': [round(v, 1) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['triangulate'] - med['triangulate_again']) / a, 4)
    out['fuse_over_triangulate'] = round(med['fuse'] / a, 4)          # < 1: asking for the fusion costs that share
    out['fuse_extra_us_per_call'] = round((1 / med['fuse'] - 1 / a) * 1e6, 1)
    return out


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if any(word in name for word in ('view_fusion', 'triangulate', 'heat_')):
                rows[name] = {'calls': int(r['Calls']), 'average_ns': float(r['AverageNs'])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one short window per arm (profiler runs)')
    ap.add_argument('--grids', default='8,16', help='grid points per axis, comma-separated')
    ap.add_argument('--stats-csv', action='append', default=[], metavar='GRID=FILE',
                    help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --quick --grids GRID')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('view_fusion_probe: no HIP device visible (there is nothing to measure on a CPU)')
    dev = torch.device('cuda', 0)
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    sk, n = spec.skeleton, PERSONS * CAMERAS
    result = {'config': 'resnet_v2_50 stride 16 h36m f16', 'device': torch.cuda.get_device_name(0), 'persons': PERSONS, 'cameras': CAMERAS,
              'grids': {}}
    eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=1)).to(dev)
    rig = rig_inputs(spec, dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    bufs = dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head))
    ref = eng.forward(x).clone()
    assert eng._heat_chunk() >= n, 'the probe times one bound forward per call'
    for grid in [int(g) for g in opts.grids.split(',')]:
        fusion = MH.fusion_params(grid=grid)
        got = eng.forward_view_fusion(x, rig['places'], rig['rows'], rig['starts'], PERSONS, rig['mirror'], fusion, 'covariance')
        assert torch.equal(got[0], ref), 'poses changed with the view fusion bound'
        iters = 2 if opts.quick else 32
        result['grids'][str(grid)] = calls_per_s(eng, x, rig, bufs, fusion, 1 if opts.quick else 5, iters)
        result['grids'][str(grid)]['joints_with_rows'] = round(float((got[5][..., 0] > 0).float().mean()), 4)
    eng.close()
    for item in opts.stats_csv:
        grid, path = item.split('=', 1)
        result.setdefault('kernels', {})[grid] = kernel_rows(path)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
