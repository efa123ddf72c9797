"""Pairs of tensors (A, B) that the caches' keys before graph.tensor_stamp could not tell apart: same address, same
element count (or shape), same `_version`, different logical contents.  Each generator builds its pair on the device it
is given and asserts ITSELF that (1) the legacy key of the site it is meant for is equal for A and B, (2) the contents
differ, (3) both are valid inputs of that site.  A torch change that ends a collision then fails here, loudly, instead
of leaving a test that compares a tensor with itself.

Scenarios
    stride       a prefix `buf[:n]` against every second element `buf[::2]` of one buffer
    transposed   `pairs.t()` of an [E, 2] tensor against `pairs.view(2, E)`   (codes: a square [R, R] tensor)
    dtype        an int64 tensor against the int32 view of its first half, with the same element count

One-element index tensors have no colliding pair and none is generated: every view that starts at the same address reads
element 0 of the buffer, and on a little-endian machine the low word (or byte) of a valid index IS that index, so stride,
shape and dtype cannot change what a one-element view lists.  Length 1 is covered by the hit, update and eviction cases
of the cache tests instead.

The int32 view of int64 indices reads (low word, high word) pairs: every second element is 0.  Where a site wants unique
indices (the identity nodes of mark_ids / id_branch) the dtype pair therefore has three elements, [a, 0, b] against
[a, b, c]; where repeats are allowed (select_rows, edge lists, codes) it has the full length.
"""
import torch


def legacy_index_key(t):
    """CSRGraph.select_rows / mark_ids / id_branch and the ego shortcut, before tensor_stamp"""
    return (t.data_ptr(), t.numel(), t._version)


def legacy_shape_key(t):
    """layers.get_graph / seed_graph_cache (with num_nodes next to it), encoders.cached_codes and ops' one-hot caches"""
    return (t.data_ptr(), tuple(t.shape), t._version)


def _checked(A, B, key, lo, hi, what):
    assert key(A) == key(B), f"{what}: the legacy key no longer collides: {key(A)} != {key(B)}"
    assert A.shape == B.shape, what
    assert not torch.equal(A.to(torch.int64), B.to(torch.int64)), f"{what}: A and B list the same elements"
    for t in (A, B):
        assert not t.is_floating_point() and int(t.min()) >= lo and int(t.max()) < hi, f"{what}: out of [{lo}, {hi})"
    return A, B


def _perm(n, high, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(high, generator=g)[:n]


# --------------------------------------------------------------------------------------------------- 1-D index tensors
def index_pair(scenario, device, n, high, unique=True, dtype=torch.int64, seed=0):
    """(A, B): 1-D index tensors of n elements in [0, high); without repeats when `unique`"""
    what = f"index {scenario} n={n}"
    if scenario == "stride":
        assert n >= 2 and 2 * n <= high
        buf = _perm(2 * n, high, seed).to(dtype).to(device)
        A, B = buf[:n], buf[::2]
        assert A.stride() == (1,) and B.stride() == (2,)
        assert torch.equal(A.cpu(), buf.cpu()[:n]) and torch.equal(B.cpu(), buf.cpu()[0:2 * n:2])
    elif scenario == "dtype":
        assert dtype == torch.int64 and n >= 2 and (not unique or n <= 3)
        vals = _perm(n, high - 1, seed) + 1                       # no 0 among them: the high words supply the zeros
        A = vals.to(device)
        B = A.view(torch.int32)[:n]
        assert B.dtype == torch.int32
        want = torch.stack([vals, torch.zeros_like(vals)], 1).reshape(-1)[:n]      # little-endian (low, high) words
        assert torch.equal(B.cpu().long(), want)
    else:
        raise ValueError(scenario)
    A, B = _checked(A, B, legacy_index_key, 0, high, what)
    if unique:
        for t in (A, B):
            assert torch.unique(t).numel() == n, f"{what}: repeated index"
    return A, B


def index_scenarios(n, unique=True):
    """the scenarios that have a pair at this length"""
    if n < 2:
        return ()
    return ("stride", "dtype") if (not unique or n <= 3) else ("stride",)


# ------------------------------------------------------------------------------------------------- [2, E] edge lists
def edge_pair(scenario, device, E, n_nodes, seed=0):
    """(A, B): [2, E] edge lists with node ids in [0, n_nodes).  The lists are what the asserts below say: A and B read
    as COO give different (row, col) multisets."""
    g = torch.Generator().manual_seed(1000 + seed)
    what = f"edges {scenario} E={E}"
    if scenario == "stride":
        buf = torch.randint(0, n_nodes, (2, 2 * E), generator=g)
        dev = buf.to(device)
        A, B = dev[:, :E], dev[:, ::2]
        wantA, wantB = buf[:, :E], buf[:, 0:2 * E:2]
    elif scenario == "transposed":
        pairs = torch.randint(0, n_nodes, (E, 2), generator=g)
        dev = pairs.to(device)
        A, B = dev.t(), dev.view(2, E)
        wantA = torch.stack([pairs[:, 0], pairs[:, 1]])            # edge k = the k-th pair
        wantB = pairs.reshape(-1).reshape(2, E)                    # edge k = (flat[k], flat[E + k])
    elif scenario == "dtype":
        vals = torch.randint(1, n_nodes, (2, E), generator=g)
        A = vals.to(device)
        B = A.view(torch.int32)[:, :E]
        wantA = vals
        wantB = torch.stack([vals, torch.zeros_like(vals)], 2).reshape(2, 2 * E)[:, :E]
    else:
        raise ValueError(scenario)
    assert torch.equal(A.cpu().long(), wantA) and torch.equal(B.cpu().long(), wantB), what
    assert A.shape == (2, E) and B.shape == (2, E)

    def coo(t):
        return sorted(zip(t[0].tolist(), t[1].tolist()))
    assert coo(wantA) != coo(wantB), f"{what}: the same edges"
    return _checked(A, B, legacy_shape_key, 0, n_nodes, what)


EDGE_SCENARIOS = ("stride", "transposed", "dtype")


# ---------------------------------------------------------------------------------------- [R, K] integer code tensors
def code_pair(scenario, device, R, K, dim, dtype=torch.int64, seed=0):
    """(A, B): [R, K] integer codes, every column in [0, dim)"""
    g = torch.Generator().manual_seed(2000 + seed)
    what = f"codes {scenario} [{R}, {K}]"
    if scenario == "stride":
        buf = torch.randint(0, dim, (R, 2 * K), generator=g).to(dtype)
        dev = buf.to(device)
        A, B = dev[:, :K], dev[:, ::2]
        wantA, wantB = buf[:, :K], buf[:, 0:2 * K:2]
    elif scenario == "transposed":
        assert R == K
        sq = torch.randint(0, dim, (R, R), generator=g).to(dtype)
        dev = sq.to(device)
        A, B = dev.t(), dev.view(R, R)
        wantA, wantB = sq.t(), sq
    elif scenario == "dtype":
        assert dtype == torch.int64
        vals = torch.randint(1, dim, (R, K), generator=g)
        A = vals.to(device)
        B = A.view(torch.int32)[:, :K]
        wantA = vals
        wantB = torch.stack([vals, torch.zeros_like(vals)], 2).reshape(R, 2 * K)[:, :K]
    else:
        raise ValueError(scenario)
    assert torch.equal(A.cpu().long(), wantA.long()) and torch.equal(B.cpu().long(), wantB.long()), what
    assert A.shape == (R, K) and B.shape == (R, K)
    return _checked(A, B, legacy_shape_key, 0, dim, what)


CODE_SCENARIOS = ("stride", "transposed", "dtype")
