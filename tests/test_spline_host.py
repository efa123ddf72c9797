"""splineconv, host side (no device): the entry coefficients against the naive (b, k) formula of tests/_spline_ref.py, a
hand case through the oracle, the closure of include/mp_spline.h over the library's exports, the binding and the
poisoning cases (mirroring tests/test_centrality_host.py), the argument checks of both entries before anything is
launched, the state dict's names and shapes with the lin.weight hook, the layer's refusals and the registration."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _spline_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_spline.h")
INVALID, UNSUPPORTED, WORKSPACE = 1, 2, 3
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
U_CASES = (0.0, 2.0 ** -149, 0.25, 0.5, 1.0 - 2.0 ** -24, 1.0)


# ---- the coefficients ---------------------------------------------------------------------------------------------------

def test_entry_weights_are_the_naive_basis_summed_per_matrix():
    from graphgym_amd.splineconv import spline_entry_weights
    u = torch.tensor(U_CASES, dtype=torch.float32)
    assert u[1] > 0 and u[4] < 1                     # the subnormal and the last float below one are what they claim
    want = torch.zeros(len(U_CASES), 2)
    for b, k in R.basis(u):
        want[torch.arange(len(U_CASES)), k] += b
    for shape in ((-1,), (-1, 1)):
        got = spline_entry_weights(u.reshape(shape))
        assert got.shape == (len(U_CASES), 2) and got.dtype == torch.float32
        assert torch.equal(got, want)
        assert torch.equal(got.sum(1), torch.ones(len(U_CASES)))
    assert torch.equal(got[0], torch.tensor([1.0, 0.0])) and torch.equal(got[5], torch.tensor([0.0, 1.0]))
    assert torch.equal(got[2], torch.tensor([0.75, 0.25]))
    # outside the contract nothing indexes: a k is 0 or 1 for every finite u
    far = spline_entry_weights(torch.tensor([-0.25, 1.5, 2.0, -3.0, 1e30]))
    assert bool(torch.isfinite(far).all()) and torch.equal(far.sum(1), torch.ones(5))
    assert spline_entry_weights(torch.zeros(0, 1)).shape == (0, 2)


def test_hand_case_through_the_oracle():
    """x = [1, 2, 3], W0 = 10, W1 = 20, root = 1, bias = 0.5; edges 0 -> 2 (u = .25), 1 -> 2 (u = 1), 2 -> 0 (u = 0):
    node 0 gets 3 * 10 + 1 + .5, node 1 nothing but 2 + .5, node 2 the mean of .75 * 10 + .25 * 20 = 12.5 and 2 * 20 = 40,
    26.25, + 3 + .5"""
    x = torch.tensor([[1.0], [2.0], [3.0]])
    src, dst = torch.tensor([0, 1, 2]), torch.tensor([2, 2, 0])
    u = torch.tensor([[0.25], [1.0], [0.0]])
    weight = torch.tensor([[[10.0]], [[20.0]]])
    for dt in (torch.float32, torch.float64):
        out = R.spline_conv(x.to(dt), src, dst, u.to(dt), weight.to(dt), torch.ones(1, 1, dtype=dt),
                            torch.tensor([0.5], dtype=dt))
        assert torch.equal(out, torch.tensor([[31.5], [2.5], [29.75]], dtype=dt))
    # the same three edges as the layer sees them: one coefficient pair per edge
    from graphgym_amd.splineconv import spline_entry_weights
    assert torch.equal(spline_entry_weights(u), torch.tensor([[0.75, 0.25], [0.0, 1.0], [1.0, 0.0]]))


# ---- the header's closure -----------------------------------------------------------------------------------------------

def declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_spline_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound_and_the_reverse():
    from graphgym_amd import _lib, _lib_spline
    from graphgym_amd import build as mpbuild
    lib = _lib_spline.lib()
    names = declared_symbols()
    assert names == ["mp_spline_agg_f32", "mp_spline_fold_f32"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_spline.h but not exported"
        assert n in _lib_spline.PROTOTYPES_SPLINE, f"{n} has no ctypes prototype"
    for n in _lib_spline.PROTOTYPES_SPLINE:
        assert n.startswith("mp_spline_") and n in names, f"ctypes binds {n} which mp_spline.h does not declare"
        assert getattr(lib, n).argtypes == _lib_spline.PROTOTYPES_SPLINE[n][1]
    engine = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
    assert "mp_spline_" not in engine
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mp_spline_")]
    assert HEADER in mpbuild.HEADERS and "spmm.hip" in mpbuild.SOURCES


def test_every_entry_has_a_poisoning_case():
    """mirrors tests/test_poison_host.py::test_every_c_entry_has_a_case_or_a_reason for include/mp_spline.h"""
    import test_poison_spline_gpu as P
    from graphgym_amd import _lib_spline
    covered = set()
    for case in P.CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        covered |= set(case.entries)
    every = set(declared_symbols())
    assert every == set(_lib_spline.PROTOTYPES_SPLINE)
    assert covered == every, f"cases {sorted(covered)} against entries {sorted(every)}"


# ---- the C entries, before anything is launched -------------------------------------------------------------------------

def _call(name, N=10, d=8, ldx=None, ldy=None, ws_bytes=0, counts=(1, 0, 0, 1, 1, 320, 1024, 256), rowptr=FAKE, col=FAKE,
          w=FAKE, plan=FAKE, X=FAKE, Y=FAKE, ws=None):
    from graphgym_amd import _lib_spline
    fold = name == "mp_spline_fold_f32"
    ldx = (2 * d if fold else d) if ldx is None else ldx
    ldy = (d if fold else 2 * d) if ldy is None else ldy
    c = None if counts is None else (C.c_int32 * 8)(*counts)
    return getattr(_lib_spline.lib(), name)(rowptr, col, w, N, plan, c, X, ldx, Y, ldy, d, ws, ws_bytes, None)


@pytest.mark.parametrize("name", ["mp_spline_agg_f32", "mp_spline_fold_f32"])
def test_entries_check_their_arguments_before_any_launch(name):
    fold = name.endswith("fold_f32")
    for missing in ("rowptr", "plan", "X", "Y"):
        assert _call(name, **{missing: None}) == INVALID, missing
    assert _call(name, counts=None) == INVALID
    assert _call(name, N=-1) == INVALID and _call(name, d=0) == INVALID and _call(name, d=-4) == INVALID
    # a leading dimension below its row: X holds d (agg) or 2 d (fold) columns, Y the other
    assert _call(name, d=8, ldx=(15 if fold else 7)) == INVALID
    assert _call(name, d=8, ldy=(7 if fold else 15)) == INVALID
    assert _call(name, N=2 ** 31) == UNSUPPORTED and _call(name, N=2 ** 31 - 1) == UNSUPPORTED
    assert _call(name, d=2 ** 30) == UNSUPPORTED
    assert _call(name, counts=(0, 0, 0, 1, 1, 320, 1024, 256)) == INVALID           # a plan without a segment
    hub = (1, 1, 5, 1, 5, 320, 1024, 256)                                            # one hub row in five pieces
    assert _call(name, counts=hub, col=None) == INVALID and _call(name, counts=hub, w=None) == INVALID
    need = 5 * 8 * 4
    need = (need + 255) // 256 * 256 * (1 if fold else 2)                            # two_branch: a second slab of partials
    assert _call(name, counts=hub, ws=None, ws_bytes=0) == WORKSPACE
    assert _call(name, counts=hub, ws=FAKE, ws_bytes=need - 1) == WORKSPACE
    # nothing to do: no row, no launch (and no pointer is looked at)
    assert _call(name, N=0, X=None, Y=None, col=None, w=None) == 0


# ---- the layer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [False, True])
def test_state_dict_matches_reference_names(bias):
    from graphgym_amd.splineconv import SplineConv, SplineConvLayer
    want = {"weight": (2, 12, 32), "root": (12, 32)}
    if bias:
        want["bias"] = (32,)
    torch.manual_seed(0)
    layer = SplineConvLayer(12, 32, bias=bias)
    assert {n: tuple(v.shape) for n, v in layer.state_dict().items()} == want
    bound = 1.0 / math.sqrt(12 * 2)
    for n, v in layer.state_dict().items():
        assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.5 * bound, n
    sd = {n: tuple(v.shape) for n, v in SplineConv(12, 32, bias=bias).state_dict().items()}
    assert sd == {"model." + n: s for n, s in want.items()}
    assert "model.bias" not in SplineConv(12, 32).state_dict()                 # the wrapper's bias=False (layer.py:178)


def test_lin_weight_of_later_checkpoints_loads_as_root():
    from graphgym_amd.splineconv import SplineConv
    torch.manual_seed(1)
    m = SplineConv(5, 3, bias=True)
    sd = {"model.weight": torch.randn(2, 5, 3), "model.lin.weight": torch.randn(3, 5), "model.bias": torch.randn(3)}
    keep = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.model.root, keep["model.lin.weight"].t()) and torch.equal(m.model.weight, keep["model.weight"])
    own = SplineConv(5, 3, bias=True)
    own.load_state_dict(m.state_dict(), strict=True)                           # and the era's names as they are
    assert torch.equal(own.model.root, m.model.root)
    with pytest.raises(RuntimeError, match="lin.weight|root"):
        SplineConv(5, 3, bias=True).load_state_dict({"model.weight": keep["model.weight"], "model.bias": keep["model.bias"]})


def test_layer_refusals():
    from graphgym_amd.splineconv import SplineConvLayer
    for kw in (dict(dim=2), dict(kernel_size=3), dict(dim=3, kernel_size=5)):
        with pytest.raises(ValueError, match=r"layer\.py:180"):
            SplineConvLayer(4, 4, **kw)
    with pytest.raises(ValueError, match="order"):
        SplineConvLayer(4, 4, order="both")
    layer = SplineConvLayer(4, 4)
    x, ei = torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long)
    for ef in (None, torch.zeros(3, 2), torch.zeros(3)):
        with pytest.raises(ValueError, match=r"layer\.py:180"):
            layer(x, ei, ef)
    with pytest.raises(TypeError, match="float32 only"):
        layer(x.to(torch.bfloat16), ei, torch.zeros(3, 1, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="float32 only"):
        layer(x, ei, torch.zeros(3, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="no gradient with respect to edge_feature"):
        layer(x, ei, torch.zeros(3, 1, requires_grad=True))
    with pytest.raises(ValueError, match="3 rows"):
        layer(x, torch.zeros(2, 4, dtype=torch.long), torch.zeros(3, 1))
    from graphgym_amd._lib import EngineError
    with pytest.raises(EngineError, match="HIP device"):                       # the engine has no CPU path
        layer(x, ei, torch.zeros(3, 1))


def test_ops_refuse_cpu_tensors_other_dtypes_and_a_differentiable_w():
    from graphgym_amd import ops
    from graphgym_amd._lib import EngineError
    for fn in (ops.spline_agg, ops.spline_fold):
        with pytest.raises(EngineError, match="HIP device"):
            fn(None, torch.zeros(3, 2), torch.zeros(4, 4))
        with pytest.raises(EngineError, match="HIP device"):
            fn(None, torch.zeros(3, 2, dtype=torch.float64), torch.zeros(4, 4))


def test_key_registered_in_its_own_dictionary():
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd import registry, splineconv
    assert registry.layer_dict["splineconv"] is splineconv.SplineConv
    assert plugin.SPLINE_KEYS == {"splineconv": splineconv.SplineConv}
    for other in (plugin.ALL_KEYS, plugin.DESIGN_KEYS, plugin.EDGE_KEYS, plugin.EDGE_ATT_KEYS, plugin.OGB_KEYS):
        assert "splineconv" not in other
    assert len(plugin.ALL_KEYS) == 18
    assert plugin.install_spline() == ["splineconv"] and plugin.install_spline(override=False) == ["splineconv"]
    assert plugin.installed_spline_keys == ["splineconv"]
    with pytest.raises(KeyError, match="Key splineconv is already pre-defined."):
        registry.register_layer("splineconv", splineconv.SplineConv)
