"""Records profiles/track_prior_parity.json: the worst deviation of the track-predicted prior rows from the fp64 restatement
(tests/track_prior_ref.py) per key -- `mu` (|mu - ref| / max(1, |ref|)) and `block` (a precision block's deviation over its
largest entry) --
  gpu/<precision>/<head>         the rows a bound forward wrote (tests/test_gpu_track_prior.py), whose run also holds the posterior
                                 to the entry on the dumped logits and to the prior bind, bit for bit
Nothing gates on this file: the tests hold the bounds derived from the number formats (track_prior_ref.MU_BOUND, BLOCK_BOUND),
which are written next to the figures.

    python tools/track_prior_parity.py [--out FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import torch
    from tests import track_prior_ref as TP
    if not torch.cuda.is_available():
        raise SystemExit('track_prior_parity: no HIP device visible (the host-compiled code is held by tests/test_track_prior.py)')
    from tests import test_gpu_track_prior as TG
    rec = {'worst': TG.gpu_deviations(torch.device('cuda', 0)), 'device': torch.cuda.get_device_name(0),
           'bounds': {'mu': TP.MU_BOUND, 'block': TP.BLOCK_BOUND},
           'what': 'worst deviation of the written prior rows from the fp64 restatement per key: mu = |mu - ref| / max(1, |ref|), '
                   'block = a precision block over its largest entry; the tests assert `bounds`, not these figures'}
    out = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'track_prior_parity.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    for key in sorted(rec['worst']):
        w = rec['worst'][key]
        print(f'{key:32s} mu {w["mu"]:.3e}  block {w["block"]:.3e}')


if __name__ == '__main__':
    main(sys.argv[1:])
