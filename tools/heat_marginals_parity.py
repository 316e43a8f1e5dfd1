"""Records profiles/heat_marginals_parity.json: the worst deviation of the heat-map marginals from the fp64 restatement
(tests/heat_marginals_ref.py), absolute in probability and relative to the row's largest entry, per key --
  host/<accumulator, logits>     heat_marginals.hip's arithmetic compiled for the host (tests/test_heat_marginals.py)
  gpu/<precision>/<head>         the bound forward against the logits of the same forward (tests/test_gpu_heat_marginals.py)
  gpu/f64/golden-oracle          precision 'f64' end to end against the fp64 oracle's logits
  gpu/<accumulator, logits>      the kernel-level entry on the crafted volumes of tests/test_gpu_heat_volumes.py
The tests assert heat_marginals_ref.GATE (4) times these figures.  The reference is always the restatement or the oracle.

    python tools/heat_marginals_parity.py [--host-only | --volumes-only]

Without a GPU (or with --host-only) the gpu/ keys of an existing file are kept as they are; --volumes-only measures the
gpu/<accumulator, logits> keys alone and keeps every other key."""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import torch
    from tests import heat_marginals_ref as HR, test_heat_marginals as TH
    rec = {'worst': {}, 'smallest_voxels': {}}
    if os.path.exists(HR.PARITY):
        rec = HR.recorded()
    volumes_only = '--volumes-only' in argv
    with tempfile.TemporaryDirectory() as tmp:
        import ctypes as C
        dll = None if volumes_only else TH.compile_for_host(pathlib.Path(tmp), 'host_heat_marginals', ['heat_marginals.hip'], TH.HOST_BODY)
        if dll is not None:
            dll.host_heat_marginals.restype = C.c_int
            dll.host_heat_marginals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p]
        for key, (a, r) in (TH.host_deviations(dll) if dll is not None else {}).items():
            rec['worst'][key] = {'abs': a, 'rel': r}
            rec['smallest_voxels'][key] = min(s * s * d for s in TH.SIDES for _, d in TH.HEADS)
    if '--host-only' not in argv and torch.cuda.is_available():
        from tests import test_gpu_heat_marginals as TG, test_gpu_heat_volumes as TV
        found = {} if volumes_only else TG.gpu_deviations(torch.device('cuda', 0))
        found.update(TV.gpu_deviations(torch.device('cuda', 0), 'marginals'))
        for key, (a, r, voxels) in found.items():
            rec['worst'][key] = {'abs': a, 'rel': r}
            rec['smallest_voxels'][key] = voxels
        rec['device'] = torch.cuda.get_device_name(0)
    rec['gate'] = HR.GATE
    rec['what'] = 'worst |kernel - fp64 restatement| per key: abs in probability, rel to the largest entry of the row'
    os.makedirs(os.path.dirname(HR.PARITY), exist_ok=True)
    with open(HR.PARITY, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for key in sorted(rec['worst']):
        w = rec['worst'][key]
        print(f'{key:32s} abs {w["abs"]:.3e}  rel {w["rel"]:.3e}  one voxel {1.0 / rec["smallest_voxels"][key]:.3e}')


if __name__ == '__main__':
    main(sys.argv[1:])
