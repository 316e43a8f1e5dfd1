"""Records profiles/heat_modes_parity.json: the worst deviation of the heat-map modes from the fp64 restatement
(tests/heat_modes_ref.py) per key -- `prob` (mass and peak, in probability), `grid` (coords01, in grid steps), `cov` (cov01,
relative to one voxel's variance) --
  host/<accumulator, logits>     heat_modes.hip's kernel body compiled for the host (tests/test_heat_modes.py)
  gpu/<precision>/<head>         the bound forward against the logits of the same forward (tests/test_gpu_heat_modes.py)
  gpu/<accumulator, logits>      the kernel-level entry on the crafted volumes of tests/test_gpu_heat_volumes.py
The tests assert heat_modes_ref.GATE (4) times these figures.  The reference is always the restatement; `voxel` is compared
exactly and has no figure.

    python tools/heat_modes_parity.py [--host-only | --volumes-only] [--out FILE]

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
    from tests import heat_modes_ref as MR, test_heat_modes as TM
    rec = {'worst': {}}
    if os.path.exists(MR.PARITY):
        rec = MR.recorded()
    volumes_only = '--volumes-only' in argv
    with tempfile.TemporaryDirectory() as tmp:
        for key, dev in ({} if volumes_only else TM.host_deviations(TM.load_host(pathlib.Path(tmp)))).items():
            rec['worst'][key] = dev
    if '--host-only' not in argv and torch.cuda.is_available():
        from tests import test_gpu_heat_modes as TG, test_gpu_heat_volumes as TV
        if not volumes_only:
            rec['worst'].update(TG.gpu_deviations(torch.device('cuda', 0)))
        rec['worst'].update(TV.gpu_deviations(torch.device('cuda', 0), 'modes'))
        rec['device'] = torch.cuda.get_device_name(0)
    rec['gate'] = MR.GATE
    rec['what'] = ('worst |kernel - fp64 restatement| per key: prob = mass and peak in probability, grid = coords01 in grid steps, '
                   'cov = cov01 relative to one voxel\'s variance')
    out = argv[argv.index('--out') + 1] if '--out' in argv else MR.PARITY
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for key in sorted(rec['worst']):
        w = rec['worst'][key]
        print(f'{key:32s} prob {w["prob"]:.3e}  grid {w["grid"]:.3e}  cov {w["cov"]:.3e}')


if __name__ == '__main__':
    main(sys.argv[1:])
