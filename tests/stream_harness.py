"""The launch contract, one protocol for every entry (tests/test_gpu_streams.py): every entry enqueues ALL of its work on the
stream it is given, and returns without waiting for it.

A subject is something that can be run on a stream from two valid input sets, A (the decoy) and B (the real one), of the same
shapes and dtypes.  The protocol (`verdict`):

  1. reference   on the default stream: fill(A), run, synchronise -> want_A; the same for B -> want_B, timed with events: T.
                 want_A != want_B, or a stale read could not be told from a fresh one.
  2. arm         fill(A), every pure output filled with the sentinel byte, the device synchronised.
  3. enqueue     on a side stream s that the null stream does not wait for: a delay of D >= max(50 ms, 20 T) of spinning
                 (torch.cuda._sleep, sized once per process with events), the event delay_done, a first look at the outputs,
                 then copies of B over the working inputs and the sentinel over the pure outputs AGAIN, on s.  The first look
                 must find the armed state: whatever wrote the outputs while the delay ran did not wait for s.  The second
                 sentinel overwrites what a clear or memset that ran ahead has done, whose effect is the same for A and B.
  4. call        run(s) under torch.cuda.stream(s).  The host must be back while the delay is still running: delay_done not
                 complete and s not idle.  A delay that is over by then says nothing -- the verdict is 'synchronised' ("delay
                 too short or the call synchronised"), never a pass.
  5. compare     clones of the outputs taken on s, s synchronised: their bits must be want_B.  want_A's bits, or a mixture of
                 the two element by element, is work that ran ahead of its stream; a pure output still holding the sentinel
                 was never written.

50 ms and 20 x are conditions of the protocol, not measurements.  A and B are both valid inputs (index tensors in range in
both): a misordered launch gives a wrong answer, never an access out of range.  No retries; two streams per process at most.
The working buffers of a case are re-filled for every run, not allocated afresh: the recorded argument list points at them.

C entries are brought in by RECORDING the call an existing builder makes (`record`): while the builder runs, the entry is
replaced by a stub that keeps its argument list and launches nothing, and every device tensor whose data_ptr() the builder
takes is noted with its storage.  The working buffers of a case are the storages of the B recording -- the recorded argument
list, pointers inside host tables included, stays valid as it is -- and A and B are the bytes those storages and their
counterparts of the A recording held at the call.  What each pointer argument is comes from the prototype in the header:
`const` pointers are inputs, `*_out` / `d_out*` are pure outputs (sentinel), `*workspace* / *scratch* / *partials*` are
scratch (staged, not compared), every other pointer is updated in place: staged AND compared (the track tables, next_id, the
poses and covariance of metro_associate_tracks_rays, the bone-length table).  A storage the builder touched that no argument
points into (the planes behind a frame table) is an input."""
from __future__ import annotations

import ctypes as C
import os
import re
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('include/metro_hip.h', 'metro_pose3d_amd/csrc/experimental/metro_experimental.h')
SENTINEL_BYTE = 0xA5
MIN_DELAY_MS = 50.0
DELAY_TIMES_T = 20.0


# ---- the prototypes ---------------------------------------------------------------------------------------------------------------

@dataclass
class Param:
    name: str
    pointer: bool
    const: bool

    @property
    def role(self):
        if not self.pointer:
            return 'value'
        if self.const:
            return 'in'
        if re.search(r'workspace|scratch|partials', self.name):
            return 'scratch'
        if re.search(r'_out\d*$|^d_out', self.name):
            return 'out'
        return 'inout'


def stream_entries(root=ROOT) -> Dict[str, List[Param]]:
    """Every function of the two headers with a `void* stream` parameter -> its parameters in order."""
    found = {}
    for rel in HEADERS:
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, rel)).read(), flags=re.S)
        text = re.sub(r'//[^\n]*', '', text)
        for m in re.finditer(r'\b(metro_\w+)\s*\(([^;{()]*)\)\s*;', text):
            params = []
            for decl in m.group(2).split(','):
                decl = ' '.join(decl.split())
                name = re.search(r'(\w+)\s*(\[\s*\d*\s*\])?$', decl).group(1) if decl and decl != 'void' else ''
                params.append(Param(name, '*' in decl or '[' in decl, bool(re.match(r'const\b', decl))))
            if any(p.name == 'stream' and p.pointer for p in params):
                assert m.group(1) not in found, m.group(1)
                found[m.group(1)] = params
    return found


# ---- streams and the delay --------------------------------------------------------------------------------------------------------

_STREAMS: List[torch.cuda.Stream] = []
_VARIANT = ''
_CYCLES_PER_MS = 0.0


def _hip_runtime() -> C.CDLL:
    """The HIP runtime torch has loaded (never a second one)."""
    for line in open('/proc/self/maps'):
        path = line.split()[-1]
        if 'libamdhip64' in os.path.basename(path):
            return C.CDLL(path)
    raise RuntimeError('no libamdhip64 is mapped into this process')


def _external_nonblocking_stream(dev):
    hip = _hip_runtime()
    handle = C.c_void_p()
    with torch.cuda.device(dev):
        status = hip.hipStreamCreateWithFlags(C.byref(handle), C.c_uint(1))            # hipStreamNonBlocking = 0x01
    if status != 0 or not handle.value:
        raise RuntimeError(f'hipStreamCreateWithFlags: status {status}')
    return torch.cuda.ExternalStream(handle.value, device=dev)


def _blocks_on_the_null_stream(s, dev) -> bool:
    """True if work on the null stream waits for work queued on s (s is a blocking stream)."""
    probe = torch.zeros(16, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(MIN_DELAY_MS * cycles_per_ms(dev)))
        slept = torch.cuda.Event()
        slept.record(s)
    probe.add_(1)                                   # on the default stream, which is the null stream
    done = torch.cuda.Event()
    done.record(torch.cuda.default_stream(dev))
    done.synchronize()
    blocked = slept.query()
    s.synchronize()
    return blocked


def cycles_per_ms(dev) -> float:
    """What torch.cuda._sleep counts in, measured once with events on the default stream."""
    global _CYCLES_PER_MS
    if not _CYCLES_PER_MS:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS = cycles / max(a.elapsed_time(b), 1e-3)
    return _CYCLES_PER_MS


def side_stream(dev, second=False) -> torch.cuda.Stream:
    """The process's side stream (second: the one other stream a process may have).  EVERY stream handed out is probed: work on
    the null stream must not wait for work queued on it, or a launch that dropped its stream argument would still be ordered
    behind the delay and pass.  torch.cuda.Stream() is tried first; if the null stream is seen to wait for it (whatever the
    cause: the stream's flags, or a hardware queue it shares), a stream made with
    hipStreamCreateWithFlags(hipStreamNonBlocking) is wrapped instead and probed in turn; the variant in use is printed.  (A
    torch stream that failed the probe stays behind, idle, in torch's own pool: the harness enqueues on two streams at most.)"""
    global _VARIANT
    want = 2 if second else 1
    while len(_STREAMS) < want:
        s = None
        if _VARIANT in ('', 'torch.cuda.Stream()'):
            s = torch.cuda.Stream(dev)
            if _blocks_on_the_null_stream(s, dev):
                assert not _STREAMS, 'a second torch.cuda.Stream() fails the probe the first one passed'
                s = None
            else:
                _VARIANT = 'torch.cuda.Stream()'
        if s is None:
            _VARIANT = 'hipStreamCreateWithFlags(hipStreamNonBlocking) as torch.cuda.ExternalStream'
            s = _external_nonblocking_stream(dev)
            assert not _blocks_on_the_null_stream(s, dev), 'the null stream waits for this stream too: no side stream to test on'
        print(f'[stream_harness] side stream {len(_STREAMS) + 1}: {_VARIANT}, probed: the null stream does not wait for it')
        _STREAMS.append(s)
    assert len(_STREAMS) <= 2
    return _STREAMS[want - 1]


def stream_variant() -> str:
    return _VARIANT


# ---- subjects ---------------------------------------------------------------------------------------------------------------------

def _bytes_of(storage, dev) -> torch.Tensor:
    return torch.empty(0, dtype=torch.uint8, device=dev).set_(storage)


@dataclass
class Recording:
    entry: str
    args: list                      # as the builder passed them
    pointers: Dict[int, tuple]      # argument index -> (buffer index, byte offset)
    buffers: List[torch.Tensor]     # uint8 views of whole storages: those the arguments point into first, then the hidden ones
    roles: List[str]                # per buffer: in | inout | out | scratch
    n_pointed: int
    keep: object = None


def _pointer_value(a):
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, int):
        return a
    return None


def record(lib, entry: str, params: Sequence[Param], build: Callable[[], object]) -> Recording:
    """Runs `build` (an existing builder that ends in one call of `entry`) with the entry stubbed out; see the module docstring."""
    real = getattr(lib, entry)
    calls, noted = [], {}
    own = torch.Tensor.__dict__.get('data_ptr')
    plain = torch.Tensor.data_ptr

    def data_ptr(self):
        p = plain(self)
        if p and self.is_cuda:
            st = self.untyped_storage()
            noted.setdefault(st.data_ptr(), (st, self.device))
        return p

    def stub(*args):
        calls.append(args)
        return 0
    torch.Tensor.data_ptr = data_ptr
    setattr(lib, entry, stub)
    try:
        keep = build()
    finally:
        setattr(lib, entry, real)
        if own is None:
            del torch.Tensor.data_ptr
        else:
            torch.Tensor.data_ptr = own
    assert len(calls) == 1, f'{entry}: the builder made {len(calls)} calls of the entry, not one'
    args = list(calls[0])
    assert len(args) == len(params) == len(real.argtypes), (entry, len(args), len(params))
    torch.cuda.synchronize()
    spans = sorted((base, base + st.nbytes(), st, dev) for base, (st, dev) in noted.items() if st.nbytes())
    order, pointers, roles = [], {}, {}
    for i, (a, ty, p) in enumerate(zip(args, real.argtypes, params)):
        v = _pointer_value(a) if ty is C.c_void_p else None
        if not v or p.name == 'stream':
            continue
        hit = [s for s in spans if s[0] <= v < s[1]]
        if not hit:
            assert p.role == 'in' or not p.pointer or p.name == 'plan', f'{entry}: {p.name} points at no noted device tensor'
            continue
        base = hit[0][0]
        if base not in order:
            order.append(base)
        pointers[i] = (order.index(base), v - base)
        roles.setdefault(base, set()).add(p.role)
    n_pointed = len(order)
    order += [s[0] for s in spans if s[0] not in order]
    by_base = {s[0]: s for s in spans}
    buffers, kinds = [], []
    for base in order:
        r = roles.get(base, {'in'})
        assert len(r) == 1 or 'scratch' not in r, f'{entry}: one storage is scratch and {sorted(r)}: it would leave the comparison'
        kinds.append('inout' if 'inout' in r or (len(r) > 1 and 'scratch' not in r) else 'scratch' if 'scratch' in r else next(iter(r)))
        buffers.append(_bytes_of(by_base[base][2], by_base[base][3]))
    return Recording(entry, args, pointers, buffers, kinds, n_pointed, keep)


class RecordedCall:
    """A C entry as a subject: the B recording's argument list on the B recording's storages."""

    def __init__(self, lib, entry: str, params: Sequence[Param], rec_a: Recording, rec_b: Recording, extra_compare=(), sentinel=()):
        """extra_compare: (argument name, first byte, bytes) of regions of a scratch argument that are compared all the same.
        sentinel: names of in-place arguments the entry CLEARS before it uses them (a status word): they hold the sentinel in A
        and in B, as the pure outputs do, so that a clear which ran ahead of its stream is overwritten and missed in the end."""
        self.entry, self.fn, self.rec = entry, getattr(lib, entry), rec_b
        self.stream_arg = [p.name for p in params].index('stream')
        assert [b.numel() for b in rec_a.buffers] == [b.numel() for b in rec_b.buffers] and rec_a.roles == rec_b.roles and \
            rec_a.pointers == rec_b.pointers, f'{entry}: the A and B builders do not make the same call'
        for i, (x, y, ty) in enumerate(zip(rec_a.args, rec_b.args, self.fn.argtypes)):
            if ty is not C.c_void_p and isinstance(x, (int, float)):
                assert x == y, f'{entry}: argument {params[i].name} differs between A ({x}) and B ({y})'
        self.work = rec_b.buffers
        self.stage = {'A': [b.clone() for b in rec_a.buffers], 'B': [b.clone() for b in rec_b.buffers]}
        self.roles = list(rec_b.roles)
        names = [p.name for p in params]
        for name in sentinel:
            assert self.roles[rec_b.pointers[names.index(name)][0]] == 'inout', (entry, name)
            self.roles[rec_b.pointers[names.index(name)][0]] = 'out'
        # (buffer, first byte, bytes) of scratch regions a case wants compared all the same: a layer's tensor in a workspace
        self.extra = [(rec_b.pointers[names.index(name)][0], rec_b.pointers[names.index(name)][1] + off, nb) for name, off, nb in extra_compare]
        self.status = None

    def fill(self, which):
        for w, s, role in zip(self.work, self.stage[which], self.roles):
            if role != 'out':
                w.copy_(s, non_blocking=True)

    def poison(self):
        for w, role in zip(self.work, self.roles):
            if role == 'out':
                w.fill_(SENTINEL_BYTE)

    def run(self, stream_ptr):
        args = list(self.rec.args)
        args[self.stream_arg] = C.c_void_p(stream_ptr)
        self.status = self.fn(*args)

    def check_status(self):
        assert self.status == 0, f'{self.entry}: status {self.status}'

    def snapshot(self):
        out = [w.clone() for w, role in zip(self.work, self.roles) if role in ('out', 'inout')]
        return out + [self.work[b][off:off + nb].clone() for b, off, nb in self.extra]

    def pure(self):
        kinds = [role for role in self.roles if role in ('out', 'inout')] + ['inout'] * len(self.extra)
        return [k == 'out' for k in kinds]


class Chain:
    """A Python call as a subject: fn(*tensors) -> tensor or tuple of tensors, on device-resident inputs it does not write."""

    def __init__(self, fn, inputs_a: Sequence[torch.Tensor], inputs_b: Sequence[torch.Tensor]):
        assert [(t.shape, t.dtype) for t in inputs_a] == [(t.shape, t.dtype) for t in inputs_b]
        self.fn = fn
        self.stage = {'A': [t.clone() for t in inputs_a], 'B': [t.clone() for t in inputs_b]}
        self.work = [t.clone() for t in inputs_b]
        self.result = None

    def fill(self, which):
        for w, s in zip(self.work, self.stage[which]):
            w.copy_(s, non_blocking=True)

    def poison(self):
        self.result = None

    def run(self, stream_ptr):
        r = self.fn(*self.work)
        flat = []

        def walk(x):
            if isinstance(x, torch.Tensor):
                flat.append(x)
            elif isinstance(x, (tuple, list)):
                for y in x:
                    walk(y)
            elif isinstance(x, dict):
                for y in x.values():
                    walk(y)
        walk(r)
        assert flat, 'the chain returned no tensor'
        self.result = flat

    def check_status(self):
        pass

    def snapshot(self):
        if self.result is None:
            return []
        return [t.contiguous().reshape(-1).view(torch.uint8).clone() if t.numel() else t.reshape(-1).to(torch.uint8) for t in self.result]

    def pure(self):
        return [False] * len(self.result)


# ---- the protocol -----------------------------------------------------------------------------------------------------------------

@dataclass
class Verdict:
    kind: str                       # ok | synchronised | idle | ran-ahead | never-written | wrong-bits
    message: str
    t_ms: float = 0.0
    d_ms: float = 0.0
    detail: dict = field(default_factory=dict)

    def require_ok(self):
        assert self.kind == 'ok', f'{self.kind}: {self.message}'


def _same(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(xs, ys))


def reference_run(subject, dev, what=''):
    """Step 1: the subject on the default stream from A and from B -> (want_A, want_B, T in ms of the B run, by events)."""
    default = torch.cuda.default_stream(dev)
    assert torch.cuda.current_stream(dev) == default
    want = {}
    for which in ('A', 'B'):
        subject.fill(which)
        subject.poison()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        subject.run(0 if isinstance(subject, RecordedCall) else default.cuda_stream)
        t1.record()
        torch.cuda.synchronize(dev)
        subject.check_status()
        want[which] = subject.snapshot()
    assert not _same(want['A'], want['B']), f'{what}: inputs A and B give the same output bits: a stale read could not be told apart'
    return want['A'], want['B'], t0.elapsed_time(t1)


def verdict(subject, dev, stream: Optional[torch.cuda.Stream] = None, what='', asynchronous=True, busy=True,
            wrap: Optional[Callable] = None, reference=None) -> Verdict:
    """Runs the protocol of the module docstring on `subject`; `wrap(subject, stream)` replaces the plain call of step 4 (the
    planted faults).  asynchronous=False: an entry that synchronises by contract -- step 4's conditions are not required, the
    ordering and the bits are.  busy=False: the stream need not still be busy when the call returns (chains that make one
    documented host synchronisation pass asynchronous=False, busy=False).  reference: (want_A, want_B, T) of an earlier run of
    the same subject, for the calls of a sequence that must all give the default-stream result."""
    s = stream if stream is not None else side_stream(dev)
    default = torch.cuda.default_stream(dev)
    assert torch.cuda.current_stream(dev) == default
    # 1. reference
    ref = reference if reference is not None else reference_run(subject, dev, what)
    want, t_ms = {'A': ref[0], 'B': ref[1]}, ref[2]
    if isinstance(subject, Chain):
        # a chain allocates its outputs: one call on s beforehand (on the decoy) leaves the blocks it needs in that stream's pool
        # of the caching allocator, so that the call under test does not have to ask the runtime for memory
        subject.fill('A')
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(s):
            subject.run(s.cuda_stream)
        s.synchronize()
        subject.result = None
    # 2. arm
    subject.fill('A')
    subject.poison()
    armed = subject.snapshot()
    torch.cuda.synchronize(dev)
    # 3. enqueue
    d_ms = max(MIN_DELAY_MS, DELAY_TIMES_T * t_ms)
    cycles = int(1.25 * d_ms * cycles_per_ms(dev))
    with torch.cuda.stream(s):
        begun = torch.cuda.Event(enable_timing=True)
        begun.record(s)
        host_begun = time.perf_counter()
        torch.cuda._sleep(cycles)
        delay_done = torch.cuda.Event(enable_timing=True)
        delay_done.record(s)
        early = subject.snapshot()          # what the outputs hold when the delay ends: anything but the armed state ran ahead
        subject.fill('B')
        subject.poison()                    # the sentinel again, ON s: a clear that ran ahead of the stream is overwritten here
        # 4. call
        if wrap is None:
            subject.run(s.cuda_stream)
        else:
            wrap(subject, s)
        returned_early = not delay_done.query()
        still_busy = not s.query()
        # 5. compare
        got = subject.snapshot()
    delay_done.synchronize()
    host_ms = (time.perf_counter() - host_begun) * 1e3
    s.synchronize()
    torch.cuda.synchronize(dev)
    subject.check_status()
    # D by the two events, and by the host's clock from the enqueue of the delay on the idle stream to the end of the delay (an
    # upper estimate by the launch latency; of an entry that synchronises by contract, by the rest of the call too).  The pair of
    # events has been seen to read 18.9 ms for a delay of the same cycle count that reads 62.4 ms in every other case (around
    # the capture of a forward, on a torch pool stream); the delay counts a constant-rate clock, so the larger figure holds.
    by_events = begun.elapsed_time(delay_done)
    measured = max(by_events, host_ms)
    print(f'[stream] {what}: T = {t_ms:.3f} ms, D = {measured:.1f} ms (events {by_events:.1f} ms, host {host_ms:.1f} ms, asked {d_ms:.1f} ms) '
          f'on {_VARIANT or "the given stream"}')
    v = lambda kind, msg: Verdict(kind, f'{what}: {msg}', t_ms, measured, dict(want=want, got=got, early=early))
    if measured < d_ms:
        return v('synchronised', f'delay too short ({measured:.1f} ms of {d_ms:.1f} ms)')
    if asynchronous and not returned_early:
        return v('synchronised', 'delay too short or the call synchronised: the delay in front of the call was over when it returned')
    if asynchronous and busy and not still_busy:
        return v('idle', 'the stream was idle when the call returned')
    if not _same(early, armed):
        if _same(early, want['A']):
            return v('ran-ahead', "work ran ahead of its stream: while the delay still ran the outputs got the decoy's bits (want_A)")
        changed = sum(int((x != y).sum()) for x, y in zip(early, armed))
        return v('ran-ahead', f'work ran ahead of its stream: {changed} output bytes were written while the delay in front of the call still ran')
    if _same(got, want['B']):
        return v('ok', 'the bits of the default-stream run')
    if _same(got, want['A']):
        return v('ran-ahead', "work ran ahead of its stream: the outputs have the decoy's bits (want_A)")
    flat = lambda xs: torch.cat([x.reshape(-1) for x in xs]) if xs else torch.empty(0, dtype=torch.uint8, device=dev)
    g, a, b = flat(got), flat(want['A']), flat(want['B'])
    if g.shape == b.shape and bool(((g == a) | (g == b)).all()):
        return v('ran-ahead', f'work ran ahead of its stream: a mixture of want_A and want_B ({int((g != b).sum())} of {g.numel()} bytes are want_A\'s)')
    untouched = [i for i, (x, p) in enumerate(zip(got, subject.pure())) if p and x.numel() and bool((x == SENTINEL_BYTE).all())]
    if untouched:
        return v('never-written', f'never written: output buffer(s) {untouched} still hold the sentinel')
    return v('wrong-bits', f'{int((g != b).sum()) if g.shape == b.shape else "all"} of {g.numel()} output bytes differ from the default-stream run')
