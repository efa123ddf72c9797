"""The harness of tests/test_grad_subsets_gpu.py: one autograd formula, run with exactly a given subset of its inputs
as `requires_grad` leaves, against a float64 / float32 CPU evaluation of the same formula (tests/_tol.py: both).

`run` checks the forward result(s) and every requested gradient (rows through `close`, parameter gradients and scalar
losses through `close_all`), that every input keeps its bits, and that no input outside the subset received a `.grad`.
It returns the engine's results so that a caller can hold them bit for bit against the all-inputs run."""
import torch

from _layout import Unchanged, same_bits
from _tol import both, close, close_all, mag_of

def subsets(names):
    """every non-empty subset of `names` (in their order), the full set first"""
    names = tuple(names)
    out = [tuple(n for i, n in enumerate(names) if m >> i & 1) for m in range(1, 1 << len(names))]
    return sorted(out, key=lambda s: -len(s))


def relu_like(pre, y_engine):
    """differentiate the reference through the engine's own ReLU pattern (an input within rounding of zero has an arbitrary
    subgradient), after checking that the two patterns agree wherever |pre| > 1e-5 max |pre|"""
    mask = y_engine > 0
    p = pre.detach()
    far = p.abs() > 1e-5 * float(p.abs().max())
    assert bool(((p > 0) == mask)[far].all()), "activation pattern differs away from zero"
    return pre * mask.to(pre.dtype)


def hub_graph(dev, N=400, E=5000, hub=1500, seed=21, weighted=True, **build):
    """(G, rows, cols, val, ei): edges source -> destination with `hub` entries forced into destination 3 (a hub row
    above the default hub_deg, a hub column once transposed) and one row in twenty receiving nothing; rows / cols /
    val: the operator's entries in CSR order on the CPU"""
    import graphgym_amd as ga
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    if hub:
        ei[1, :hub] = 3
    ei = ei[:, ei[1] % 20 != 7]
    w = torch.rand(ei.size(1), generator=g) + 0.2 if weighted else None
    G = ga.CSRGraph.from_edge_index(ei.to(dev), N, None if w is None else w.to(dev), **build)
    return G, G.row_ids().cpu().long(), G.col.cpu().long(), (None if G.val is None else G.val.cpu()), ei


def _rows(t, param=False):
    """a scalar as one row of one element; a per-node vector as one row per node"""
    if t is None:
        return None
    if t.dim() == 0:
        return t.reshape(1)
    return t[:, None] if (t.dim() == 1 and not param) else t


def _lay(dy, layout, dev):
    """the incoming gradient in the given memory layout on the device"""
    if layout == "slice":                 # a column slice of a wider buffer
        wide = torch.randn(dy.size(0), dy.size(1) + 7, generator=torch.Generator().manual_seed(5))
        wide[:, 3:3 + dy.size(1)] = dy
        v = wide.to(dev)[:, 3:3 + dy.size(1)]
        assert v.stride(0) == dy.size(1) + 7
        return v
    if layout == "transposed":
        v = dy.t().contiguous().to(dev).t()
        assert v.stride() == (1, dy.size(0))
        return v
    assert layout == "contig"
    return dy.to(dev)


def _backward(outs, dys, used, cast):
    torch.autograd.backward([outs[i] for i in used], [cast(dys[i]) for i in used])


def run(op, inputs, oracle, subset, dys, dev, params=(), mags=None, what="", layout="contig", scalar_loss=False,
        **tol):
    """op(d) -> tensor or tuple, d the named inputs on the device (None stays None); oracle(c, t, eng) the same formula on
    the CPU leaves t (cast by c), eng the engine's forward results on the CPU (for its ReLU pattern); subset: the names
    that require a gradient; dys: one incoming gradient per output, None for an output the loss does not use; layout:
    "contig" | "slice" | "transposed" | "expand" (the loss is the plain sum: the gradient arrives as an expanded scalar);
    mags: {name or "y": float64 bound} or a function of eng returning one (tests/_tol.py rule (d))"""
    dys = tuple(dys) if isinstance(dys, (tuple, list)) else (dys,)
    used = [i for i, g in enumerate(dys) if g is not None]
    assert subset and all(inputs[k] is not None for k in subset)
    d = {k: (None if v is None else v.detach().clone().to(dev).requires_grad_(k in subset))
         for k, v in inputs.items()}
    with Unchanged(*[v.detach() for v in d.values() if v is not None]):
        outs = op(d)
        outs = (outs,) if isinstance(outs, torch.Tensor) else tuple(outs)
        if layout == "expand":
            sum(outs[i].sum() for i in used).backward()
        else:
            _backward(outs, dys, used, lambda g: _lay(g, layout, dev))
    eng = [o.detach().cpu() for o in outs]

    def ref(c):
        t = {k: (None if v is None else c(v).detach().clone().requires_grad_(k in subset)) for k, v in inputs.items()}
        o = oracle(c, t, eng)
        o = (o,) if isinstance(o, torch.Tensor) else tuple(o)
        if layout == "expand":
            sum(o[i].sum() for i in used).backward()
        else:
            _backward(o, dys, used, c)
        return [v.detach() for v in o] + [t[k].grad for k in subset]
    r64, r32 = both(ref)
    mags = mags(eng) if callable(mags) else (mags or {})
    n = len(eng)
    for i, o in enumerate(eng):
        name = "y" if n == 1 else f"y{i}"
        if scalar_loss:
            close_all(_rows(o), (_rows(r64[i]), _rows(r32[i])), what=f"{what} {subset} {name}")
        else:
            kw = dict(tol)
            if mags.get(name) is not None:
                kw["mag"] = _rows(mags[name])
            close(_rows(o), (_rows(r64[i]), _rows(r32[i])), what=f"{what} {subset} {name}", **kw)
    for j, k in enumerate(subset):
        got = d[k].grad
        assert got is not None and got.shape == d[k].shape and got.dtype == d[k].dtype, f"{what} {subset}: d{k}"
        refs = (r64[n + j], r32[n + j])
        if k in params:
            close_all(got, refs, what=f"{what} {subset} d{k}")
        else:
            kw = dict(tol)
            if mags.get(k) is not None:
                kw["mag"] = _rows(mags[k])
            close(_rows(got), (_rows(refs[0]), _rows(refs[1])), what=f"{what} {subset} d{k}", **kw)
    # (autograd itself never fills the .grad of a tensor that does not require one, so this holds whatever the formula
    # returns; an unneeded launch or buffer shows only to a spy: test_no_masked_gradient_without_an_input_gradient)
    for k, v in d.items():
        assert v is None or k in subset or v.grad is None, f"{what} {subset}: {k} received a gradient"
    res = {("y" if n == 1 else f"y{i}"): o.detach() for i, o in enumerate(outs)}
    res.update({k: d[k].grad for k in subset})
    return res


def abs_mags(oracle, inputs, dys, eng=None):
    """{"y": ..., name: ...}: the float64 evaluation of the oracle and of every gradient on the ABSOLUTE values of all float
    inputs, constants and the incoming gradient — the sums of absolute terms of results that cancel (rule (d))"""
    names = [k for k, v in inputs.items() if v is not None]

    def ref(c):
        ca = lambda v: c(v).abs() if (isinstance(v, torch.Tensor) and v.is_floating_point()) else c(v)   # noqa: E731
        t = {k: (None if v is None else ca(v).detach().clone().requires_grad_(True)) for k, v in inputs.items()}
        o = oracle(ca, t, eng)
        o.backward(ca(dys))
        return [o.detach()] + [t[k].grad for k in names]
    r = mag_of(ref)
    return dict(zip(["y"] + names, r))


def hold_bits(full, res, names, what):
    """the named results of a subset run equal the all-inputs run bit for bit"""
    for k in names:
        if k in res and k in full:
            assert same_bits(res[k], full[k]), f"{what}: {k} differs from the all-inputs run"


def sweep(op, inputs, oracle, dys, dev, names=None, bits=(), **kw):
    """`run` on every non-empty subset of `names` (default: every input that is present), the full set first; the results
    named in `bits` are held bit for bit against the full run.  Returns the full run's results."""
    names = [k for k, v in inputs.items() if v is not None] if names is None else names
    full = None
    for s in subsets(names):
        res = run(op, inputs, oracle, s, dys, dev, **kw)
        if full is None:
            full = res
        else:
            hold_bits(full, res, bits, f"{kw.get('what', '')} {s}")
    return full
