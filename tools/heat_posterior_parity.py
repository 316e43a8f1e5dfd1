"""Records profiles/heat_posterior_parity.json: the worst deviation of the heat-map posterior from the fp64 restatement
(tests/heat_posterior_ref.py) per key -- `logev` (log_evidence, absolute), `peak` (peak', in probability), `grid` (coords01', in
grid steps), `cov` (cov01', in units of one voxel's variance) --
  host/<accumulator, logits>     heat_posterior.hip's kernel body compiled for the host (tests/test_heat_posterior.py)
  gpu/<precision>/<head>         the bound forward against the logits of the same forward (tests/test_gpu_heat_posterior.py)
  gpu/<accumulator, logits>      the kernel-level entry on the crafted volumes of tests/test_gpu_heat_volumes.py
The tests assert heat_posterior_ref.GATE (4) times these figures (the host's fp64 instantiations: 1e-12 instead).  The reference
is always the restatement.

    python tools/heat_posterior_parity.py [--host-only | --volumes-only] [--out FILE]

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
    from tests import heat_posterior_ref as PR, test_heat_posterior as TP
    rec = {'worst': {}}
    if os.path.exists(PR.PARITY):
        rec = PR.recorded()
    volumes_only = '--volumes-only' in argv
    with tempfile.TemporaryDirectory() as tmp:
        for key, dev in ({} if volumes_only else TP.host_deviations(TP.load_host(pathlib.Path(tmp)))).items():
            rec['worst'][key] = dev
    if '--host-only' not in argv and torch.cuda.is_available():
        from tests import test_gpu_heat_posterior as TG, test_gpu_heat_volumes as TV
        if not volumes_only:
            rec['worst'].update(TG.gpu_deviations(torch.device('cuda', 0)))
        rec['worst'].update(TV.gpu_deviations(torch.device('cuda', 0), 'posterior'))
        rec['device'] = torch.cuda.get_device_name(0)
    rec['gate'] = PR.GATE
    rec['what'] = ('worst |kernel - fp64 restatement| per key: logev = log_evidence (absolute), peak = peak\' in probability, '
                   'grid = coords01\' in grid steps, cov = cov01\' in units of one voxel\'s variance')
    out = argv[argv.index('--out') + 1] if '--out' in argv else PR.PARITY
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for key in sorted(rec['worst']):
        w = rec['worst'][key]
        print(f'{key:32s} ' + '  '.join(f'{m} {w[m]:.3e}' for m in PR.MEASURES))


if __name__ == '__main__':
    main(sys.argv[1:])
