"""Layer-level parity on the GPU: every layer_type key the engine serves, forward and
backward, against the committed golden records (tests/golden/layers.npz, produced by the
oracle's restatement of TfgIDLayer.py / idconv.py / the PyG and tf_geometric layers).

The records carry the weights under the names of the reference's parameters, so loading
them also checks that ours are named and shaped alike.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from _tol import assert_close_all, assert_close_rows

F_IN, D = 8, 16
TOL = 1e-5   # north_star's bar, per output row, against the float64 evaluation of the oracle (tests/_tol.py)


def close_out(a, z, key):
    """layer outputs / input gradients: per row, 1e-5 of the row's magnitude in the float64 record, or twice the
    fp32 oracle's own distance from it"""
    assert_close_rows(a, z[key + "64"], TOL, ref32=z[key], what=key)


def close_grad(a, z, key):
    """parameter gradients (reductions over all nodes): one scale per tensor; key is '<layer>/grad/<name>'"""
    assert_close_all(a, z[key.replace("/grad/", "/grad64/")], TOL, ref32=z[key], what=key)


def mlp2():
    return nn.Sequential(nn.Linear(F_IN, D), nn.ReLU(), nn.Linear(D, D))


def set_mlp(seq, z, key, prefix):
    with torch.no_grad():
        seq[0].weight.copy_(torch.from_numpy(z[f"{key}/param/{prefix}.0"]).t())
        seq[0].bias.copy_(torch.from_numpy(z[f"{key}/param/{prefix}.1"]))
        seq[2].weight.copy_(torch.from_numpy(z[f"{key}/param/{prefix}.2"]).t())
        seq[2].bias.copy_(torch.from_numpy(z[f"{key}/param/{prefix}.3"]))


def check_mlp_grads(seq, z, key, prefix):
    close_grad(seq[0].weight.grad.t(), z, f"{key}/grad/{prefix}.0")
    close_grad(seq[0].bias.grad, z, f"{key}/grad/{prefix}.1")
    close_grad(seq[2].weight.grad.t(), z, f"{key}/grad/{prefix}.2")
    close_grad(seq[2].bias.grad, z, f"{key}/grad/{prefix}.3")


def load_named(mod, z, key, names, transpose=()):
    with torch.no_grad():
        for n in names:
            p = mod
            for part in n.split("."):
                p = getattr(p, part)
            src = torch.from_numpy(z[f"{key}/param/{n}"])
            if n in transpose:
                src = src.t()
            assert p.shape == src.shape, (key, n, p.shape, src.shape)
            p.copy_(src)


def check_named_grads(mod, z, key, names, transpose=()):
    for n in names:
        p = mod
        for part in n.split("."):
            p = getattr(p, part)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        if n in transpose:
            g = g.t()
        close_grad(g, z, f"{key}/grad/{n}")


@pytest.fixture(scope="module")
def rec(golden):
    return golden("layers.npz")


def run(layer_call, z, key, dev):
    x = torch.from_numpy(z["x"]).to(dev).requires_grad_(True)
    out = layer_call(x)
    dy = torch.from_numpy(z["dy"]).to(dev)[:, :out.size(1)]
    out.backward(dy)
    close_out(out, z, f"{key}/out")
    close_out(x.grad, z, f"{key}/grad_x")


@pytest.mark.parametrize("order", ["transform_first", "aggregate_first"])
def test_gcnidconv(dev, rec, order):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.GCNIDConvLayer(F_IN, D, bias=True, order=order).to(dev)
    names = ["weight", "weight_id", "bias"]
    load_named(m, rec, "gcnidconv", names)
    run(lambda x: m(x, ei, ids), rec, "gcnidconv", dev)
    check_named_grads(m, rec, "gcnidconv", names)


@pytest.mark.parametrize("agg", ["add", "mean", "max"])
def test_idconv_and_generalconv(dev, rec, agg):
    from graphgym_amd import layers as L
    from graphgym_amd.config import cfg
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    old = (cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg)
    try:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = agg, False, "concat"
        m = L.GeneralIDConvLayer(F_IN, D, bias=True, order="transform_first").to(dev)
        names = ["weight", "weight_id", "bias"]
        load_named(m, rec, f"idconv_{agg}", names)
        run(lambda x: m(x, ei, ids), rec, f"idconv_{agg}", dev)
        check_named_grads(m, rec, f"idconv_{agg}", names)
        m = L.GeneralConvLayer(F_IN, D, bias=True).to(dev)
        names = ["weight", "weight_self", "bias"]
        load_named(m, rec, f"generalconv_{agg}", names)
        run(lambda x: m(x, ei), rec, f"generalconv_{agg}", dev)
        check_named_grads(m, rec, f"generalconv_{agg}", names)
    finally:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = old


def test_sageidconv(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.SAGEIDConvLayer(F_IN, D, bias=True, concat=True).to(dev)
    names = ["weight", "weight_id", "bias"]
    load_named(m, rec, "sageidconv", names)
    run(lambda x: m(x, ei, ids), rec, "sageidconv", dev)
    check_named_grads(m, rec, "sageidconv", names)


def test_gatidconv(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.GATIDConvLayer(F_IN, D, bias=True).to(dev)
    names = ["weight", "weight_id", "att", "bias"]
    load_named(m, rec, "gatidconv", names)
    run(lambda x: m(x, ei, ids), rec, "gatidconv", dev)
    check_named_grads(m, rec, "gatidconv", names)


def test_ginidconv_and_ginconv(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.GINIDConvLayer(mlp2(), mlp2()).to(dev)
    set_mlp(m.nn, rec, "ginidconv", "nn")
    set_mlp(m.nn_id, rec, "ginidconv", "nn_id")
    run(lambda x: m(x, ei, ids), rec, "ginidconv", dev)
    check_mlp_grads(m.nn, rec, "ginidconv", "nn")
    check_mlp_grads(m.nn_id, rec, "ginidconv", "nn_id")
    m = L.GINConvLayer(mlp2()).to(dev)
    set_mlp(m.nn, rec, "ginconv", "nn")
    run(lambda x: m(x, ei), rec, "ginconv", dev)
    check_mlp_grads(m.nn, rec, "ginconv", "nn")


@pytest.mark.parametrize("order", ["transform_first", "aggregate_first"])
def test_gcnconv(dev, rec, order):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    m = L.GCNConvLayer(F_IN, D, bias=True, order=order).to(dev)
    load_named(m, rec, "gcnconv", ["weight", "bias"])
    run(lambda x: m(x, ei), rec, "gcnconv", dev)
    check_named_grads(m, rec, "gcnconv", ["weight", "bias"])


def test_sageconv(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    m = L.SAGEConvLayer(F_IN, D, bias=True).to(dev)
    names = ["lin_l.weight", "lin_l.bias", "lin_r.weight"]
    load_named(m, rec, "sageconv", names)
    run(lambda x: m(x, ei), rec, "sageconv", dev)
    check_named_grads(m, rec, "sageconv", names)


def test_gatconv(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    m = L.GATConvLayer(F_IN, D, bias=True).to(dev)
    with torch.no_grad():
        m.lin_l.weight.copy_(torch.from_numpy(rec["gatconv/param/weight"]).t())
        m.att_r.copy_(torch.from_numpy(rec["gatconv/param/att_dst"]).view(1, 1, D))
        m.att_l.copy_(torch.from_numpy(rec["gatconv/param/att_src"]).view(1, 1, D))
        m.bias.copy_(torch.from_numpy(rec["gatconv/param/bias"]))
    run(lambda x: m(x, ei), rec, "gatconv", dev)
    close_grad(m.lin_l.weight.grad.t(), rec, "gatconv/grad/weight")
    close_grad(m.att_r.grad.view(1, D), rec, "gatconv/grad/att_dst")
    close_grad(m.att_l.grad.view(1, D), rec, "gatconv/grad/att_src")
    close_grad(m.bias.grad, rec, "gatconv/grad/bias")


# ---- TF family ----------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["transform_first", "aggregate_first"])
def test_tf_idgcn_and_gcn(dev, rec, order):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.IDGCN(D, activation="relu", in_features=F_IN, order=order).to(dev)
    names = ["kernel", "kernel_id", "bias"]
    load_named(m, rec, "tf_idgcn", names)
    run(lambda x: m([x, ei, ids]), rec, "tf_idgcn", dev)
    check_named_grads(m, rec, "tf_idgcn", names)
    m = L.GCN(D, activation=torch.relu, in_features=F_IN, order=order).to(dev)
    load_named(m, rec, "tf_gcn", ["kernel", "bias"])
    run(lambda x: m([x, ei, None]), rec, "tf_gcn", dev)
    check_named_grads(m, rec, "tf_gcn", ["kernel", "bias"])


def test_tf_idsage_and_sage(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.IDSAGE(D, activation=torch.relu, in_features=F_IN).to(dev)
    names = ["self_kernel", "id_kernel", "neighbor_kernel", "bias"]
    load_named(m, rec, "tf_idsage", names)
    run(lambda x: m([x, ei, ids]), rec, "tf_idsage", dev)
    check_named_grads(m, rec, "tf_idsage", names)
    m = L.MeanGraphSage(D, activation=torch.relu, in_features=F_IN).to(dev)
    names = ["self_kernel", "neighbor_kernel", "bias"]
    load_named(m, rec, "tf_sage", names)
    run(lambda x: m([x, ei]), rec, "tf_sage", dev)
    check_named_grads(m, rec, "tf_sage", names)
    with pytest.raises(Exception):
        L.IDSAGE(7, concat=True)                                   # odd units (TfgIDLayer.py:42-43)


def test_tf_idgin_and_gin(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.IDGIN(mlp2(), mlp2()).to(dev)
    set_mlp(m.mlp_model, rec, "tf_idgin", "mlp")
    set_mlp(m.mlp_id, rec, "tf_idgin", "mlp_id")
    run(lambda x: m([x, ei, ids, None]), rec, "tf_idgin", dev)
    check_mlp_grads(m.mlp_model, rec, "tf_idgin", "mlp")
    check_mlp_grads(m.mlp_id, rec, "tf_idgin", "mlp_id")
    m = L.GIN(mlp2()).to(dev)
    set_mlp(m.mlp_model, rec, "tf_gin", "mlp")
    run(lambda x: m([x, ei, None]), rec, "tf_gin", dev)
    check_mlp_grads(m.mlp_model, rec, "tf_gin", "mlp")


@pytest.mark.parametrize("heads", [1, 4])
def test_tf_idgat(dev, rec, heads):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    m = L.IDGAT(D, activation="relu", num_heads=heads, in_features=F_IN).to(dev)
    names = ["query_kernel", "query_bias", "key_kernel", "key_bias", "kernel", "kernel_id", "bias"]
    key = f"tf_idgat_h{heads}"
    load_named(m, rec, key, names)
    run(lambda x: m([x, ei, ids]), rec, key, dev)
    check_named_grads(m, rec, key, names)


def test_tf_gat(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    m = L.GAT(D, activation="relu", in_features=F_IN).to(dev)
    names = ["query_kernel", "query_bias", "key_kernel", "key_bias", "kernel", "bias"]
    load_named(m, rec, "tf_gat", names)
    run(lambda x: m([x, ei]), rec, "tf_gat", dev)
    check_named_grads(m, rec, "tf_gat", names)


# ---- the GraphGym boundary: layer_dict[key](dim_in, dim_out, bias=...)(batch) ---------------
def test_registered_keys_run_on_a_batch(dev, rec):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd.registry import layer_dict
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    for key in plugin.ALL_KEYS:
        layer = layer_dict[key](F_IN, D, bias=True).to(dev)
        batch = types.SimpleNamespace(node_feature=torch.from_numpy(rec["x"]).to(dev), edge_index=ei,
                                      node_id_index=ids)
        out = layer(batch)
        assert out is batch and batch.node_feature.shape == (int(rec["n"]), D), key
        assert torch.isfinite(batch.node_feature).all(), key
        batch.node_feature.sum().backward()
        # one CSR per self-loop policy was cached on the batch and is reused by the next layer
        assert hasattr(batch, "_mp_graph_cache"), key


def test_cached_layer_raises_on_changed_edge_count(dev, rec):
    from graphgym_amd import layers as L
    ei = torch.from_numpy(rec["edge_index"]).to(dev)
    ids = torch.from_numpy(rec["node_id_index"]).to(dev)
    x = torch.from_numpy(rec["x"]).to(dev)
    m = L.GCNIDConvLayer(F_IN, D, cached=True).to(dev)
    m(x, ei, ids)
    with pytest.raises(RuntimeError, match="Cached"):
        m(x, ei[:, :-2], ids)                                       # idconv.py:157-163


@pytest.mark.parametrize("agg", ["add", "mean", "max"])
def test_generalconv_with_edge_features(dev, agg):
    """message = x_j + edge_feature (generalconv.py:99-106): per-entry messages reduced on the aggregation kernel,
    forward and the gradients to x, the weights and the edge features, against the oracle in float64"""
    from graphgym_amd import layers as L
    from graphgym_amd.config import cfg
    from oracle import ref_layers as RL
    g = torch.Generator().manual_seed(9)
    n, E = 300, 2500
    ei = torch.randint(0, n, (2, E), generator=g)
    x = torch.randn(n, F_IN, generator=g)
    ef = torch.randn(E, D, generator=g)
    up = torch.randn(n, D, generator=g)
    old = (cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg)
    try:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = agg, False, "concat"
        torch.manual_seed(2)
        m = L.GeneralConvLayer(F_IN, D, bias=True).to(dev)
        xd, efd = x.to(dev).requires_grad_(True), ef.to(dev).requires_grad_(True)
        out = m(xd, ei.to(dev), edge_feature=efd)
        out.backward(up.to(dev))
        from _tol import both

        def ref_fn(c):
            xr, efr = c(x).clone().requires_grad_(True), c(ef).clone().requires_grad_(True)
            W, Ws, b = (c(p.detach().cpu()).clone().requires_grad_(True) for p in (m.weight, m.weight_self, m.bias))
            ref = RL.general_conv(xr, ei, W, Ws, b, agg=agg, edge_feature=efr)
            ref.backward(c(up))
            return ref.detach(), xr.grad, efr.grad, W.grad
        r64, r32 = both(ref_fn)
        assert_close_rows(out, r64[0], 1e-5, ref32=r32[0], what="out")
        assert_close_rows(xd.grad, r64[1], 1e-5, ref32=r32[1], what="dx")
        assert_close_rows(efd.grad, r64[2], 1e-5, ref32=r32[2], what="d edge_feature")
        assert_close_all(m.weight.grad, r64[3], 1e-5, ref32=r32[3], what="dW")
    finally:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = old


@pytest.mark.parametrize("dst_row", [1, 0])
def test_edge_features_on_a_seeded_holder(dev, dst_row):
    """layers.seed_graph_cache puts the CSR an ego expansion wrote under the keys of both edge_index conventions; its
    `eid` must be the entry positions of the convention asked for, or a gather `edge_feature[g.eid]` reads the reverse
    edge's features.  GeneralConv with edge features (dst_row = 1) and the same message passing under dst_row = 0 —
    forward and the gradients to x, the weight and the edge features — equal what an unseeded holder gives.  So does
    the TF GCN without renormalisation (loops told apart by eid < 0 under dst_row = 0)."""
    from graphgym_amd import graphgen, harness as H, layers as L, ops
    from graphgym_amd.config import cfg
    from graphgym_amd.ego import ego_batch
    import graphgym_amd as ga
    n = 4000
    base = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(n, 3, seed=8, device=dev), n)
    cen = torch.randint(0, n, (48,), generator=torch.Generator().manual_seed(3)).to(dev)
    gen = torch.Generator().manual_seed(4)
    old = (cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg)
    try:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = "add", False, "concat"
        torch.manual_seed(5)
        m = L.GeneralConvLayer(F_IN, D, bias=True).to(dev)
        for loops in ("none", "add"):
            ei, orig, ids, _, g = ego_batch(base, cen, 2, csr=loops)
            assert g is not None and g.symmetric
            n2, E = orig.numel(), ei.size(1)
            x0, ef0 = torch.randn(n2, F_IN, generator=gen).to(dev), torch.randn(E, D, generator=gen).to(dev)
            up = torch.randn(n2, D, generator=gen).to(dev)
            results = []
            for seeded in (True, False):
                holder = H.Batch()
                if seeded:
                    L.seed_graph_cache(holder, ei, n2, g, loops)
                x, ef = x0.clone().requires_grad_(True), ef0.clone().requires_grad_(True)
                m.zero_grad()
                if loops == "none":
                    if dst_row == 1:
                        out = m(x, ei, edge_feature=ef, holder=holder)
                    else:
                        gg = L.get_graph(holder, ei, n2, dst_row=0, loops="none")
                        msg = ops.gather_rows(ops.dense_fused(x, m.weight), gg.col.long()) + ef[gg.eid.long()]
                        out = ops.spmm(gg.edge_operator(), msg, "sum")
                    out.backward(up)
                    results.append([out.detach(), x.grad, ef.grad, m.weight.grad.clone()])
                else:
                    gcn = L.IDGCN(D, activation=None, renorm=False, in_features=F_IN).to(dev)
                    if results:
                        gcn.load_state_dict(results[0][-1])
                    out = gcn([x, ei, ids], holder=holder)
                    out.backward(up)
                    results.append([out.detach(), x.grad, gcn.kernel.grad, {k: v.detach().clone() for k, v in
                                                                              gcn.state_dict().items()}])
                want = ga.CSRGraph.from_edge_index(ei, n2, dst_row=dst_row, add_self_loops=(loops == "add"))
                got = L.get_graph(holder, ei, n2, dst_row=dst_row, loops=loops)
                assert torch.equal(got.eid, want.eid), f"eid under dst_row={dst_row}, loops={loops}"
            # the output and the edge-feature gradient go through eid: bit for bit; the gradient to x is a scatter-add of
            # the messages' gradients by source (float atomics: the order of the sum varies from run to run)
            out_a, dx_a, dp_a = results[0][:3]
            out_b, dx_b, dp_b = results[1][:3]
            assert torch.equal(out_a, out_b), f"loops={loops}: the output differs from the unseeded holder's"
            assert float((dx_a - dx_b).abs().max()) <= 1e-5 * float(dx_b.abs().max()), \
                f"loops={loops}: the gradient to x differs"
            if loops == "none":
                assert torch.equal(dp_a, dp_b), "the gradient to the edge features differs"
    finally:
        cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = old
