"""TEST HELPER (not collected): what the stream-ordering tests of tests/test_gpu_streams.py are made of.

The oracle comparisons of the suite run on the null stream, where every launch is serialised with every other one; a call issued on
the wrong stream computes the right answer there.  These helpers put real work in flight on a side stream, so that such a call
computes a WRONG answer from valid data instead:

    late_input(stream, real, decoy)   a device buffer that holds `decoy` now and `real` only once `stream` has drained a delay
    late_inputs(stream, (real, decoy), ...)   the same for several arguments of one call, behind one delay
    assert_busy(stream)               the delay is still running: the test is not vacuous
    side_stream(*others)              a stream whose delay does not hold up the null stream or `others` through a shared hardware queue
    consume_on(stream, *tensors)      device results read in the order of the caller's stream, with no host synchronisation before

Importing this module needs no GPU (torch is imported inside the functions)."""
import numpy as np

# One delay = torch.cuda._sleep(DELAY_CYCLES): a single-lane spin kernel on the stream.  It occupies one wave of one compute unit, so
# work that was (wrongly) issued on another stream runs at once beside it and reads the decoy.
DELAY_CYCLES = 60_000_000
_delay_done = {}          # stream handle -> event recorded right behind its last delay


def _torch():
    import torch
    return torch


def delay(stream):
    """keeps `stream` busy with ordinary work on that stream; nothing else waits for it.

    Measured once on an MI355X, with events around the spin and a host clock around the helper (20 repetitions each):
        busy time of the spin: 0.417 us per 1000 cycles, linear from 10^6 to 1.6 * 10^7 cycles (1.669 ms at 4 * 10^6, spread under
            1 %), so one delay of DELAY_CYCLES keeps the stream busy for 25 ms;
        host time from enqueueing the delay to entering the library call (the spin launch, the copy launch, one stream query):
            median 0.027 ms, largest of 20 0.113 ms; the tiny kernel late_inputs sends to the null stream and waits for adds
            less than 0.1 ms to it.
    The delay is 900 times the median and 220 times the largest host time seen: host jitter of a shared machine does not let it run out
    (assert_busy fails the test if it ever does).  Work on another stream, the null stream included, ran beside the spin at once."""
    torch = _torch()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(DELAY_CYCLES)
        done = torch.cuda.Event()
        done.record(stream)
    _delay_done[stream.cuda_stream] = done          # what assert_busy asks: work queued behind the delay does not count as the delay


def side_stream(*others):
    """a side stream for the tests: a high-priority stream on which a delay holds up neither the null stream -- where a call issued on
    the wrong stream would run -- nor any of `others` (side streams the test already holds).  Streams share a few hardware queues
    and a queue runs its kernels one after the other, so every candidate is tried out: a short spin on it, one tiny kernel on the
    other stream, which must finish while the spin runs; the next stream of torch's pool is taken if it had to wait.  late_inputs
    checks the same again at the moment of the call."""
    torch = _torch()
    tiny = torch.zeros(1, device="cuda")
    for _ in range(32):
        st = torch.cuda.Stream(priority=-1)
        beside = all(st.cuda_stream != o.cuda_stream for o in others)
        for other in (torch.cuda.default_stream(),) + tuple(others):
            if not beside:
                break
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                torch.cuda._sleep(DELAY_CYCLES // 10)
                done = torch.cuda.Event()
                done.record(st)
            with torch.cuda.stream(other):
                tiny.add_(1)
            other.synchronize()
            beside = not done.query()
            st.synchronize()
        if beside:
            return st
    raise AssertionError("no side stream found that runs beside the given ones")


def to_dev(a):
    """numpy -> CUDA tensor with the same bits (torch has no unsigned 32 / 64-bit arithmetic types: int64 / int32 views)"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).cuda()


def late_inputs(stream, *pairs, beside=()):
    """late_input for several (real, decoy) pairs behind ONE delay: the arguments of one call (keys and values, ...) -> list of buffers

    The runtime runs its streams on a few hardware queues (four by default) and a queue runs its kernels one after the other.
    Measured on an MI355X with normal-priority side streams: in about a quarter of the cases a kernel launched on the null stream
    landed in the queue of the delay and ran only after it -- a call issued on the null stream by mistake then reads the real input
    and shows nothing (it was the whole reason why a fifth of these tests could not fail).  So after the delay and the copies are
    queued, one tiny kernel goes to the null stream (and to every stream of `beside`: the streams a later call of the test is made
    under) and must finish while the delay still runs; in 48 of 48 trials that told exactly whether the next null-stream launch
    read the decoy.  If it had to wait, the helper fails: the stream is unfit (use side_stream()).
    The helper starts with a wait for the whole device: work that an earlier step of the same test left pending on any stream has run
    before the buffers are set up (a test that needs such work pending must queue it after its late inputs)."""
    torch = _torch()
    null = torch.cuda.default_stream()
    assert stream.cuda_stream != null.cuda_stream
    reals, bufs = [], []
    with torch.cuda.stream(null):
        for real, decoy in pairs:
            real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
            assert real.shape == decoy.shape and real.dtype == decoy.dtype, (real.shape, decoy.shape, real.dtype, decoy.dtype)
            assert real.size == 0 or not np.array_equal(real, decoy), "a decoy equal to the real input shows nothing"
            reals.append(to_dev(real))
            bufs.append(to_dev(decoy))
        tiny = torch.zeros(1, device="cuda")
    for t in reals + bufs:
        t.record_stream(stream)
    torch.cuda.synchronize()
    delay(stream)
    with torch.cuda.stream(stream):
        for buf, real_dev in zip(bufs, reals):
            buf.copy_(real_dev, non_blocking=True)
    for other in (null,) + tuple(beside):
        with torch.cuda.stream(other):
            tiny.add_(1)
        other.synchronize()
        assert not _delay_done[stream.cuda_stream].query(), "a kernel on another stream was queued behind the delay: it shares a hardware queue"
    return bufs


def late_input(stream, real, decoy, beside=()):
    """a device buffer shaped like `real` (numpy arrays of equal shape and dtype) that holds `decoy` until `stream` has run a delay
    and then `real`: the decoy is written on the default stream and waited for, then the delay and the copy of `real` are queued on
    `stream`.  The decoy is well-formed input of the same kind, so a call that reads the buffer too early -- on another stream, or
    without ordering -- computes a wrong answer from valid memory; it never faults.  beside: see late_inputs."""
    return late_inputs(stream, (real, decoy), beside=beside)[0]


def assert_busy(stream):
    """the condition that keeps a test from passing vacuously: the delay queued on `stream` has not finished (the delay itself: a
    stream whose delay is over and whose copies are still pending is busy, but no longer holds anything back)"""
    done = _delay_done.get(stream.cuda_stream)
    assert done is not None and not stream.query() and not done.query(), "the delay on the side stream ran out before the call under test was made"


def consume_on(stream, *tensors):
    """clones device results on `stream` with no host synchronisation in between, then synchronises and returns host copies (numpy;
    None and host arrays pass through): the results must be complete in the order of the caller's stream"""
    torch = _torch()
    with torch.cuda.stream(stream):
        clones = [t.clone() if isinstance(t, torch.Tensor) and t.is_cuda else t for t in tensors]
    stream.synchronize()
    out = [c.cpu().numpy() if isinstance(c, torch.Tensor) else c for c in clones]
    return out[0] if len(out) == 1 else out
