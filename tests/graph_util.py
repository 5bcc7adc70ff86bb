"""One capture / replay protocol for every entry point
(test_graph_capture_gpu.py, test_graph_network_gpu.py; INTEGRATION.md, "Graph
capture").

A replay skips all Python: whatever a wrapper decided, copied, cached or
converted on the host at call time is frozen into the graph.  ``captured``
therefore runs the same call three ways -- eagerly on fresh tensors, as a
capture, and as replays of that capture after its static inputs were refilled
in place -- and asks for the same bits every time:

  1. static inputs hold values A; unless ``cold``, one eager warm-up call;
  2. ``out = fn(*static)`` is captured with ``torch.cuda.graph`` on its own
     single capture stream (no side stream, no event);
  3. every output buffer is filled with the NaN pattern of sweep_util.arena,
     the graph replayed: every output element written, and bit for bit the
     eager result on A;
  4. values B are ``copy_``-ed into the static inputs, the outputs poisoned
     again, the graph replayed: bit for bit the eager result of ``fn`` on fresh
     tensors holding B;
  5. two more replays on B: the same bits;
  6. A copied back and replayed: the bits of step 3;
  7. every static input still holds, bit for bit, what was copied into it.

The eager results on A and on B (drawn from different seeds) must differ in
more than half of their elements, or the scenario fails as vacuous: a replay
that ignored the refill cannot pass step 4 by accident.  The condition is
asserted on the eager results alone, before anything is captured.  Where an
output is sparse by construction (a level gradient holds at most 2r + 2
entries per pixel row) ``judged`` names the dense outputs the condition is
asserted on; every other output must still differ somewhere -- except those
named ``constant``, which do not depend on the inputs by the call's own
definition (the network zeroes the y-flow of every prediction) and must then
be equal on A and on B.

``make``: a factory of ``fn`` for scenarios that keep Python-side state (a
block's lazily pooled levels, the stacked gate weights of gru._ZR).  Each eager
run and the capture get a fresh ``fn`` from it, so with ``cold=True`` that state
is built inside the capture and holds valid data after the first replay only
-- which is when the assertions look.

No operand of ``fn`` may be written by it: an in-place form (``z_out=z_pre``)
clones its operand inside ``fn``, which makes the clone a graph node that
re-reads the static input on every replay, and lets step 7 hold without
exception.
"""
import torch

from sweep_util import SENT16, SENT32

DEV = "cuda:0"


def _int_view(t):
    es = t.element_size()
    assert es in (2, 4), t.dtype
    return t.view(torch.int32 if es == 4 else torch.int16)


def bits(t):
    """The tensor's values as integers on the CPU (NaN payloads and the sign
    of zero count)."""
    return _int_view(t.detach()).cpu().contiguous()


def flat(out):
    """fn's result as a list of tensors (None entries dropped)."""
    if isinstance(out, torch.Tensor):
        return [out]
    res = []
    for o in out:
        if o is not None:
            res += flat(o)
    return res


def poison(outs):
    for t in outs:
        v = _int_view(t)
        v.fill_(SENT32 if v.dtype == torch.int32 else SENT16)


def same_bits(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} outputs, {len(want)} expected"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {i} is {g.shape} {g.dtype}, not " \
                                                           f"{w.shape} {w.dtype}"
        bad = int((g != w).sum())
        assert not bad, f"{what}: output {i}: {bad} of {g.numel()} elements differ"


def within(bound):
    """A comparison for ``captured(compare=)``: fp32 outputs within
    ``norm_err <= bound`` (max|a - ref| / max|ref|, golden_util.norm_err) of
    the eager result instead of bit-equal to it -- for calls whose PyTorch
    convolutions are not bit-stable between two eager runs."""
    from golden_util import norm_err

    def compare(got, want, what):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == w.dtype == torch.int32, what
            err = norm_err(g.view(torch.float32).numpy(), w.view(torch.float32).numpy())
            assert err <= bound, f"{what}: output {i}: norm_err {err:.3e} > {bound:.3e}"

    return compare


def assert_written(got, what):
    for i, g in enumerate(got):
        left = int((g == (SENT32 if g.dtype == torch.int32 else SENT16)).sum())
        assert not left, f"{what}: output {i}: {left} of {g.numel()} elements never written"


def differing(a, b, judged=None):
    """The fraction of the judged outputs' elements whose bits differ."""
    idx = range(len(a)) if judged is None else judged
    n = sum(a[i].numel() for i in idx)
    d = sum(int((a[i] != b[i]).sum()) for i in idx)
    return d / max(n, 1)


def assert_discriminates(a, b, judged=None, constant=(), what="eager"):
    if judged is None:
        judged = [i for i in range(len(a)) if i not in constant]
    assert judged and not set(judged) & set(constant)
    frac = differing(a, b, judged)
    print(f"{what}: A and B differ in {frac:.3f} of the judged elements")
    assert frac > 0.5, f"vacuous: the eager results on A and B differ in {frac:.3f} of their elements only"
    for i, (x, y) in enumerate(zip(a, b)):
        if i in constant:
            assert torch.equal(x, y), f"output {i} was declared constant and differs between A and B"
        else:
            assert bool((x != y).any()), f"vacuous: output {i} is the same on A and on B"


def eager(fn, inputs):
    """``fn`` on fresh device tensors holding ``inputs``: the outputs' bits."""
    fresh = [t.to(DEV) for t in inputs]
    keep = [bits(t) for t in fresh]
    out = flat(fn(*fresh))
    torch.cuda.synchronize()
    same_bits([bits(t) for t in fresh], keep, "eager call: an input was modified")
    return [bits(t) for t in out], [t.stride() for t in out]


def captured(fn, inputs_a, inputs_b, cold=False, make=None, judged=None, constant=(), compare=same_bits,
             warmups=1):
    """The protocol of the module docstring.  ``inputs_a`` / ``inputs_b``:
    lists of CPU tensors of the same shapes and dtypes.  ``compare``: how a
    replay's outputs are held against the eager ones (bit equality unless a
    caller has a written-down reason, see ``within``); the static inputs are
    always compared bit for bit.  ``warmups``: eager warm-up calls before the
    capture (none when ``cold``).  Returns the eager outputs' bits on A and B."""
    assert len(inputs_a) == len(inputs_b)
    assert all(a.shape == b.shape and a.dtype == b.dtype and a.device.type == "cpu"
               for a, b in zip(inputs_a, inputs_b))
    new = make if make is not None else (lambda: fn)
    want_a, strides_a = eager(new(), inputs_a)
    want_b, _ = eager(new(), inputs_b)
    assert_discriminates(want_a, want_b, judged, constant)

    static = [t.to(DEV) for t in inputs_a]                       # step 1
    run = new()
    for _ in range(0 if cold else warmups):
        run(*static)
        torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # step 2
        outs = flat(run(*static))
    assert [t.stride() for t in outs] == strides_a, "the captured call laid its outputs out differently"

    def replay(what, want):
        poison(outs)
        graph.replay()
        torch.cuda.synchronize()
        got = [bits(t) for t in outs]
        assert_written(got, what)
        compare(got, want, what)

    def refill(values):
        for s, v in zip(static, values):
            s.copy_(v)

    replay("first replay (A) against the eager call", want_a)    # step 3
    refill(inputs_b)                                             # step 4
    replay("replay after the refill with B against the eager call on B", want_b)
    same_bits([bits(s) for s in static], [bits(t) for t in inputs_b], "a static input changed (B)")
    for k in (2, 3):                                             # step 5
        replay(f"replay {k} on B", want_b)
    refill(inputs_a)                                             # step 6
    replay("replay after A was copied back", want_a)
    same_bits([bits(s) for s in static], [bits(t) for t in inputs_a], "a static input changed (A)")   # step 7
    return want_a, want_b
