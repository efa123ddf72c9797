"""SHA-256 digests of every output of every mp_bn_* / mp_dropout_keyed_f32 entry over a table of small cases, as JSON: run
once per tree in a fresh process, the two files are compared byte for byte.

    python scripts/bn_bits.py OUT.json [--root DIR]      # DIR: the tree whose package is loaded (default: this one)

Inputs are seeded on the CPU; every buffer handed in as an output is torch.empty.  The table is built from the smallest
shapes at which each path first exists (N: 2, a second statistics workgroup, more than 64 rows per workgroup; d: scalar,
vector, two column tiles; the CONCAT width pairs; an offset base, a padded row; affine or not; every kind; three T; dskip
and dslope asked for or not; the ReLU entries with and without the forward's output).  For every call the script works
out, from csrc/bn_kernels.h's dispatch, which instantiation of the three kernel templates runs, and asserts at the end
that the table reached every one."""
import ctypes as C, hashlib, itertools, json, os, sys

root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(root))
import torch
from graphgym_amd._lib import check, lib, ptr

dev = torch.device("cuda:0")
NONE, RELU, LRELU, PRELU, ELU, SELU, SILU = range(7)
PRM = {NONE: 0.0, RELU: 0.0, LRELU: 0.01, PRELU: 0.0, ELU: 1.0, SELU: 0.0, SILU: 0.0}
PLAIN, SUM, CONCAT = 0, 1, 2            # the kernels' FORM; the entries' mode is FORM - 1
ZX, ZXS, ZY = 0, 1, 2
EPS, SEED, OFFSET = 1e-5, 0x1234567, 3
hashers, rows, reached, group = {}, {}, set(), None
gen = torch.Generator().manual_seed(20240)


def rnd(*shape, shift=0.0):
    return torch.randn(*shape, generator=gen) + shift


def view(cpu, N, d, layout):
    """an [N, d] device view (layout: "", "offset": base one float past a 16-byte boundary, "stride": rows of d + 4) holding
    cpu's values, or uninitialised memory when cpu is None"""
    ld = d + 4 if layout == "stride" else d
    off = 1 if layout == "offset" else 0
    buf = torch.empty(N * ld + off, device=dev)
    v = buf[off:off + N * ld].view(N, ld)[:, :d]
    if cpu is not None:
        v.copy_(cpu)
    return v


def vec_(cpu):
    return None if cpu is None else cpu.to(dev)


def ws_for(name, N, d):
    nb = C.c_size_t(0)
    check(getattr(lib(), name)(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


def record(case, **outs):
    """case = "<table row>/<call>".  One digest per GROUP of rows (a kind, affine or not, a T: the file stays small), over
    the row, call and output names and the bytes of every output of every call of every row of the group"""
    torch.cuda.synchronize()
    rows.setdefault(group, set()).add(case.split("/")[0])
    h = hashers.setdefault(group, hashlib.sha256())
    for k, v in outs.items():
        if v is not None:
            h.update(f"{case}.{k}:".encode())
            h.update(v.contiguous().cpu().numpy().tobytes())


def vec4(d, lds, ts):
    return d % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def ld_(t):
    return 0 if t is None else t.stride(0)


def reach_fwd(act, drop, form, x, skip, out, mean, d, ds):
    vx = vec4(d, [ld_(x)], [x, mean])
    vo = vec4(4, [ld_(out)], [out])
    vs = skip is not None and vec4(ds, [ld_(skip)], [skip]) and vo
    vr = vx and vo and (form != CONCAT or ds % 4 == 0)
    if form == PLAIN:
        w = (4, 4) if vr else (1, 1)
    elif form == SUM:
        w = (4, 4) if vx and vs else (1, 1)
    else:
        w = (4 if vs else 1, 4 if vr else 1)
    reached.add(("fwd",) + w + (form, act, drop))


def reach_bwd(act, drop, x, dyr, dx, s, gout, beta, mean, d, zsrc):
    needz = act != NONE and zsrc != ZY
    w = 4 if vec4(d, [ld_(x), ld_(dyr), ld_(dx), ld_(s), ld_(gout)], [x, dyr, dx, s, gout, beta if needz else None, mean]) else 1
    reached.add(("stats", w, act, zsrc, drop))
    reached.add(("apply", w, NONE, ZX, drop) if gout is not None else ("apply", w, act, zsrc, drop))


def zsrc_of(act, drop, y, summed):
    if drop or act > RELU:
        return ZXS
    return ZY if y is not None else ZXS if summed else ZX


def expected():
    e = set()
    for act, drop in itertools.product(range(7), (False, True)):
        for w in (1, 4):
            e.add(("fwd", w, w, PLAIN, act, drop))
            e.add(("fwd", w, w, SUM, act, drop))
            e.add(("apply", w, NONE, ZX, drop))
        for ws, wx in itertools.product((1, 4), (1, 4)):
            e.add(("fwd", ws, wx, CONCAT, act, drop))
    for w in (1, 4):
        for k in ("stats", "apply"):
            for act in range(7):
                e.add((k, w, act, ZXS, True))
                if act > RELU:
                    e.add((k, w, act, ZXS, False))
            for z in (ZX, ZXS, ZY):
                e.add((k, w, RELU, z, False))
            e.add((k, w, NONE, ZX, False))
    return e


def run(N, d, layout, act, affine, T, form, ds, want_dskip, want_dslope, skip_layout=None):
    """one forward and one backward through the entries of (act, T): the *_act entries (T None) or the *_drop_* entries;
    for NONE / RELU without mask also the entries that predate the activations"""
    drop = T is not None
    case = f"N{N}_d{d}_{layout or 'plain'}_a{act}_{'aff' if affine else 'noaff'}_T{T}_f{form}_ds{ds}_k{int(want_dskip)}{int(want_dslope)}_{skip_layout}"
    assert case not in rows.get(group, ()), case
    x = view(rnd(N, d, shift=1.5), N, d, "offset" if skip_layout == "x offset" else layout)
    gamma, beta = (vec_(rnd(d) * 0.5 + 1.0), vec_(rnd(d))) if affine else (None, None)
    slope = torch.tensor([0.25], device=dev) if act == PRELU else None
    skip = view(rnd(N, ds), N, ds, "offset" if skip_layout == "offset" else layout) if form != PLAIN else None
    wo = ds + d if form == CONCAT else d
    dy = view(rnd(N, wo), N, wo, layout)
    mean, invstd, var = (torch.empty(d, device=dev) for _ in range(3))
    out = view(None, N, wo, layout)
    L = lib()
    wsn = "mp_bn_drop_ws_bytes" if drop else "mp_bn_act_ws_bytes"
    ws, nb = ws_for(wsn, N, d)
    key = (T, SEED, OFFSET) if drop else ()
    sfx = "drop_" if drop else ""
    if form == PLAIN:
        check(getattr(L, f"mp_bn_train_fwd_{sfx}act_f32")(ptr(x), ld_(x), N, d, ptr(gamma), ptr(beta), EPS, act, PRM[act], ptr(slope), *key,
                                                          ptr(out), ld_(out), ptr(mean), ptr(invstd), ptr(var), ptr(ws), nb, None))
    else:
        check(getattr(L, f"mp_bn_train_fwd_{sfx}skip_act_f32")(ptr(x), ld_(x), ptr(skip), ld_(skip), N, d, ds, form - 1, ptr(gamma), ptr(beta), EPS,
                                                               act, PRM[act], ptr(slope), *key, ptr(out), ld_(out), ptr(mean), ptr(invstd),
                                                               ptr(var), ptr(ws), nb, None))
    reach_fwd(act, drop, form, x, skip, out, mean, d, ds)
    record(case + "/fwd", out=out, mean=mean, invstd=invstd, var=var)
    dx = view(None, N, d, layout)
    dskip = view(None, N, ds, layout) if form != PLAIN and want_dskip else None
    dgamma, dbeta = (torch.empty(d, device=dev), torch.empty(d, device=dev)) if affine else (None, None)
    dslope = torch.empty(1, device=dev) if act == PRELU and want_dslope else None
    ws, nb = ws_for(wsn, N, d)
    if form == PLAIN:
        check(getattr(L, f"mp_bn_train_bwd_{sfx}act_f32")(ptr(dy), ld_(dy), ptr(x), ld_(x), N, d, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), act,
                                                          PRM[act], ptr(slope), *key, ptr(dx), ld_(dx), ptr(dgamma), ptr(dbeta), ptr(dslope),
                                                          ptr(ws), nb, None))
    else:
        check(getattr(L, f"mp_bn_train_bwd_{sfx}skip_act_f32")(ptr(dy), ld_(dy), ptr(x), ld_(x), ptr(skip), ld_(skip), N, d, ds, form - 1, ptr(gamma),
                                                               ptr(beta), ptr(mean), ptr(invstd), act, PRM[act], ptr(slope), *key, ptr(dx),
                                                               ld_(dx), ptr(dskip), ld_(dskip), ptr(dgamma), ptr(dbeta), ptr(dslope), ptr(ws),
                                                               nb, None))
    summed = form == SUM and act != NONE
    dyr = dy[:, ds:] if form == CONCAT else dy
    reach_bwd(act, drop, x, dyr, dx, skip if summed else None, dskip if summed else None, beta, mean, d, zsrc_of(act, drop, None, summed))
    wrote_dskip = dskip is not None and act != NONE      # without activation d skip is dy itself: nothing is written
    record(case + "/bwd", dx=dx, dskip=dskip if wrote_dskip else None, dgamma=dgamma, dbeta=dbeta, dslope=dslope)
    if drop or act > RELU:
        return
    # ---- the entries with the run-time relu flag and the forward's output ---------------------------------------------
    relu = int(act == RELU)
    out2 = view(None, N, wo, layout)
    ws, nb = ws_for("mp_bn_ws_bytes", N, d)
    if form == PLAIN:
        check(L.mp_bn_train_fwd_f32(ptr(x), ld_(x), N, d, ptr(gamma), ptr(beta), EPS, relu, ptr(out2), ld_(out2), ptr(mean), ptr(invstd), ptr(var),
                                    ptr(ws), nb, None))
    else:
        check(L.mp_bn_train_fwd_skip_f32(ptr(x), ld_(x), ptr(skip), ld_(skip), N, d, ds, form - 1, ptr(gamma), ptr(beta), EPS, relu, ptr(out2),
                                         ld_(out2), ptr(mean), ptr(invstd), ptr(var), ptr(ws), nb, None))
    reach_fwd(act, False, form, x, skip, out2, mean, d, ds)
    record(case + "/fwd_legacy", out=out2, mean=mean, invstd=invstd, var=var)
    if form == CONCAT:
        return
    for given in ((False, True) if relu else (False,)):      # the forward's output handed in, or NULL
        y = out2 if given else None
        dx2 = view(None, N, d, layout)
        ws, nb = ws_for("mp_bn_ws_bytes", N, d)
        if form == PLAIN:
            check(L.mp_bn_train_bwd_f32(ptr(dy), ld_(dy), ptr(y), ld_(y), ptr(x), ld_(x), N, d, ptr(gamma), ptr(mean), ptr(invstd), ptr(dx2), ld_(dx2),
                                        ptr(dgamma), ptr(dbeta), ptr(ws), nb, None))
            g = None
        else:
            g = view(None, N, d, layout) if given else None
            check(L.mp_bn_train_bwd_skip_f32(ptr(dy), ld_(dy), ptr(y), ld_(y), ptr(x), ld_(x), N, d, ptr(gamma), ptr(mean), ptr(invstd), ptr(dx2),
                                             ld_(dx2), ptr(g), ld_(g), ptr(dgamma), ptr(dbeta), ptr(ws), nb, None))
        reach_bwd(RELU if given else NONE, False, x, dy, dx2, y, g, None, mean, d, ZY if given else ZX)
        record(case + f"/bwd_legacy_y{int(given)}", dx=dx2, dskip=g, dgamma=dgamma, dbeta=dbeta)
    if form == PLAIN and relu:
        dx3 = view(None, N, d, layout)
        ws, nb = ws_for("mp_bn_ws_bytes", N, d)
        check(L.mp_bn_train_bwd_relu_f32(ptr(dy), ld_(dy), ptr(x), ld_(x), N, d, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dx3), ld_(dx3),
                                         ptr(dgamma), ptr(dbeta), ptr(ws), nb, None))
        reach_bwd(RELU, False, x, dy, dx3, None, None, beta, mean, d, ZX)
        record(case + "/bwd_legacy_relu", dx=dx3, dgamma=dgamma, dbeta=dbeta)


SHAPES = [(2, 1, ""), (2, 4, ""), (65, 3, ""), (65, 8, ""), (65, 8, "offset"), (65, 8, "stride"), (131, 260, ""),
          (131, 260, "offset"), (137, 1028, "")]
# CONCAT (d_skip, d): the four pairs of widths — the odd ones all take the 1 | 1 kernel, since no row of the [N, d_skip + d]
# output is aligned then — and the aligned pair with a skip operand that is not (the 1 | 4 kernel) or an x that is not (4 | 1)
PAIRS = [(4, 8, None), (3, 8, None), (4, 5, None), (3, 5, None), (4, 8, "offset"), (4, 8, "x offset")]
TS = (None, 0, 19661, 65536)
for act, affine, T in itertools.product(range(7), (True, False), TS):
    group = f"act{act}_{'affine' if affine else 'plain'}_T{T}"
    for N, d, layout in SHAPES:
        run(N, d, layout, act, affine, T, PLAIN, 0, False, affine)
        for want in (True, False):
            run(N, d, layout, act, affine, T, SUM, d, want, want)
    for (ds, d, sl), want in itertools.product(PAIRS, (True, False)):
        run(65, d, "", act, affine, T, CONCAT, ds, want, want, sl)
group = "dropout_keyed"
for (N, d, layout), T in itertools.product(SHAPES, TS[1:]):
    x, out = view(rnd(N, d), N, d, layout), view(None, N, d, layout)
    check(lib().mp_dropout_keyed_f32(ptr(x), ld_(x), N, d, T, SEED, OFFSET, ptr(out), ld_(out), None))
    record(f"dropout_keyed_N{N}_d{d}_{layout or 'plain'}_T{T}", out=out)

missing = expected() - reached
assert not missing and reached <= expected(), (sorted(missing), sorted(reached - expected()))
digests = {k: f"{h.hexdigest()} over {len(rows[k])} rows" for k, h in hashers.items()}
summary = {"instantiations_reached": len(reached), "rows": sum(len(v) for v in rows.values()), "groups": len(digests)}
with open(sys.argv[1], "w") as f:
    json.dump(dict(summary, digests=digests), f, indent=0, sort_keys=True)
print(json.dumps(summary))
