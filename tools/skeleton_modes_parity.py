"""Records profiles/skeleton_modes_parity.json: the worst deviation of the bound forward's skeleton outputs from the fp64
restatement (tests/skeleton_modes_ref.py) on the hand-filled cases of tests/test_gpu_skeleton_modes.py, per key
gpu/<precision>/<dataset>/<case>: `prob` (the marginals, in probability) and `logs` (log_evidence and log_map, absolute).  The
device's outputs are fp32, so a figure holds the kernel's fp64 deviation and the one rounding to fp32.  `choice` and
`coords01_sel` are compared exactly and have no figure.  The tests hold the bounds of skeleton_modes_ref.compare, not this record.

    python tools/skeleton_modes_parity.py [--out FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARITY = os.path.join(ROOT, 'profiles', 'skeleton_modes_parity.json')


def main(argv):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('skeleton_modes_parity: no HIP device visible')
    from metro_pose3d_amd import _lib
    from tests import test_gpu_skeleton_modes as TG
    cuda, lib = torch.device('cuda', 0), _lib.load()
    rec = {'worst': {}, 'device': torch.cuda.get_device_name(0),
           'what': 'worst |fp32 output - fp64 restatement| per key: prob = the marginals in probability, logs = log_evidence and '
                   'log_map, absolute'}
    for precision in ('f16', 'f64'):
        for dataset in ('h36m', 'merged'):
            for name, (prob, logs) in TG.hand_deviations(cuda, lib, precision, dataset).items():
                rec['worst'][f'gpu/{precision}/{dataset}/{name}'] = {'prob': prob, 'logs': logs}
    out = argv[argv.index('--out') + 1] if '--out' in argv else PARITY
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for key in sorted(rec['worst']):
        w = rec['worst'][key]
        print(f'{key:40s} prob {w["prob"]:.3e}  logs {w["logs"]:.3e}')


if __name__ == '__main__':
    main(sys.argv[1:])
