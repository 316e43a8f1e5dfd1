#!/usr/bin/env python3
"""What asking for the track-predicted posterior costs, and that not asking costs nothing.

    python tools/track_prior_probe.py [--out FILE] [--quick]              # one JSON object on stdout (and in FILE)

RN50 stride 16 h36m (synthetic weights), f16, at 64 and 256 crops.  Three arms INTERLEAVED window by window in one process:
plain (Engine.forward), bound (Engine.forward_track_posterior on a table of 64 tracks: the head also stores its fp32 logits, the
track_priors launch, the heat_posterior launch, three small output tensors allocated per call), plain again.
The two plain arms are the same code on the same data: their relative difference (`aa_spread`) is the noise margin the bound
arm has to be read against.  Crops/s from a host clock around `iters` forwards that end in a synchronisation, after 3 warm-up
windows, median of 5 windows.  Nothing gates on these figures.
Per-launch times of the new kernel come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/track_prior_probe.py --quick --batches 64
(one batch per run: the table averages over all launches of a kernel), and `--stats-csv 64=<dir>/.../*_kernel_stats.csv`
(repeatable) folds that table's track_priors / heat_posterior rows into the JSON under `kernels`.
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

from metro_pose3d_amd import ModelSpec, synth  # noqa: E402
from metro_pose3d_amd.engine import Engine  # noqa: E402

N_TRACKS = 64


def track_inputs(spec, n, dev):
    """A table of N_TRACKS persons 3.5 to 5.5 m in front of the crops' cameras and one slot, time and record per crop."""
    from tests import track_prior_ref as TP
    case = TP.random_case(TP.Head(spec), n, N_TRACKS, 'camera', 'root', 1, seed=2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(state=up(np.asarray(case['state'], np.float64)), slot=up(np.asarray(case['slot'], np.int32)),
                times=up(np.nan_to_num(np.asarray(case['times'], np.float64), nan=10.02)),
                records=up(np.ascontiguousarray(case['records']).view(np.uint8).reshape(n, -1)),
                mirror=up(np.asarray(spec.skeleton.out_mirror, np.int32)))


def crops_per_s(eng, x, track, bufs, windows, iters):
    n = x.shape[0]
    plain = lambda: eng.forward(x, out=bufs['poses'])
    bound = lambda: eng.forward_track_posterior(x, coords='camera', depth='root', out=bufs['poses'], coords01=bufs['coords01'], **track)
    arms = (('plain', plain), ('bound', bound), ('plain_again', plain))
    res = {k: [] for k, _ in arms}
    for w in range(3 + windows):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            if w >= 3:
                res[name].append(n * iters / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in res.items()}
    a = 0.5 * (med['plain'] + med['plain_again'])
    out = {k: {'median': round(med[k], 1), 'windows': [round(v, 1) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['plain'] - med['plain_again']) / a, 4)
    out['bound_over_plain'] = round(med['bound'] / a, 4)          # < 1: asking for the posterior costs that share
    out['bound_extra_us_per_call'] = round((n / med['bound'] - n / a) * 1e6, 1)
    return out


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if 'track_priors' in name or 'heat_posterior' in name:
                rows[name] = {'calls': int(r['Calls']), 'average_ns': float(r['AverageNs'])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one short window per arm (profiler runs)')
    ap.add_argument('--batches', default='64,256', help='crops per call, comma-separated')
    ap.add_argument('--stats-csv', action='append', default=[], metavar='BATCH=FILE',
                    help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --quick --batches BATCH')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_prior_probe: no HIP device visible (there is nothing to measure on a CPU)')
    dev = torch.device('cuda', 0)
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=0, logit_gain=synth.logit_gain_for(50, 16))
    sk = spec.skeleton
    result = {'config': 'resnet_v2_50 stride 16 h36m f16', 'device': torch.cuda.get_device_name(0), 'tracks': N_TRACKS, 'batches': {}}
    for n in [int(b) for b in opts.batches.split(',')]:
        eng = Engine(spec, params, 'f16', max_batch=n, device=dev)
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=1)).to(dev)
        track = track_inputs(spec, n, dev)
        bufs = {'poses': torch.empty((n, sk.n_out, 3), device=dev), 'coords01': torch.empty((n, sk.n_head, 3), device=dev)}
        ref = eng.forward(x).clone()
        poses, post, _, reason = eng.forward_track_posterior(x, coords='camera', depth='root', coords01=bufs['coords01'], **track)
        assert torch.equal(poses, ref), 'poses changed with the track prior bound'
        assert bool(torch.isfinite(post).all()), 'a posterior of the probe is not finite'
        assert eng._heat_chunk() == n, 'the probe times one bound forward per call'
        iters = 2 if opts.quick else max(4, 2048 // n)
        result['batches'][str(n)] = crops_per_s(eng, x, track, bufs, 1 if opts.quick else 5, iters)
        result['batches'][str(n)]['scratch_bytes'] = int(eng.lib.metro_plan_prior_scratch_bytes(eng._plan, n))
        result['batches'][str(n)]['rows_with_a_prior'] = round(float((reason == 0).float().mean()), 4)
        eng.close()
    for item in opts.stats_csv:
        batch, path = item.split('=', 1)
        result.setdefault('kernels', {})[batch] = kernel_rows(path)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
