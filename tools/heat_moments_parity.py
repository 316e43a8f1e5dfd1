"""Measures the fp32-accumulator parity figure of the heat-map moments on the GPU and writes profiles/heat_moments_parity.json
(or --out): for every fp32 case of tests/test_gpu_heat_moments.py, the largest deviation of a Cov01 entry from the fp64
restatement of the kernel's own logits, relative to max(entry scale, the variance of one voxel).  The tests assert four times
the recorded maximum.   python tools/heat_moments_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'heat_moments_parity.json'))
    opts = ap.parse_args()
    import torch
    from metro_pose3d_amd import _lib
    from tests import test_gpu_heat_moments as T
    cases = T.fp32_deviations(_lib.load(), torch.device('cuda', 0))
    rec = dict(what='largest |Cov01 entry - fp64 restatement| / max(sqrt(var_a var_b), (1/(S-1))^2/12), fp32 accumulators',
               device=torch.cuda.get_device_name(0), max_relative_deviation=max(cases.values()), cases=cases)
    os.makedirs(os.path.dirname(opts.out), exist_ok=True)
    with open(opts.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
