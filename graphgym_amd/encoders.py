"""GraphGym's integer-feature encoders on the engine: graphgym/models/feature_encoder.py

    IntegerFeatureEncoder   'Integer'      feature_encoder.py:13-31    encoder.weight
    SingleAtomEncoder       'SingleAtom'   feature_encoder.py:34-53    atom_type_embedding.weight
    AtomEncoder             'Atom'         feature_encoder.py:56-81    atom_embedding_list.{i}.weight
    BondEncoder             'Bond'         feature_encoder.py:84-103   bond_embedding_list.{i}.weight

Constructors, parameter names and the xavier_uniform_ initialisation follow the reference, so state dicts interchange.
The forward is one ops.embed_sum launch on the K tables stacked into one [C, d] operand (torch.cat of the separate
parameters: autograd splits the table gradient); the additions run in the reference's order, so the result has the bits
of its fp32 loop.  The int32 copy of a batch's codes is made — and checked against the tables, IndexError as
nn.Embedding raises — once per batch and cached on it next to the graph cache.
"""
import torch
import torch.nn as nn

from . import ops
from .graph import tensor_stamp

# The feature dims of ogb.utils.features.get_atom_feature_dims() / get_bond_feature_dims(), used when ogb is not
# importable.  These are the values of ogb 1.x as recalled from the library; no copy of ogb was at hand to confirm
# them.
ATOM_FEATURE_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
BOND_FEATURE_DIMS = [5, 6, 2]

try:
    from ogb.utils.features import get_atom_feature_dims, get_bond_feature_dims
    full_atom_feature_dims = list(get_atom_feature_dims())
    full_bond_feature_dims = list(get_bond_feature_dims())
except Exception:
    full_atom_feature_dims = list(ATOM_FEATURE_DIMS)
    full_bond_feature_dims = list(BOND_FEATURE_DIMS)


def table_offsets(dims):
    """row offsets of K tables of `dims` rows stacked into one"""
    off, at = [], 0
    for d in dims:
        off.append(at)
        at += int(d)
    return off


def cached_codes(holder, field, codes, dims, make=None):
    """the checked int32 form of `codes` (a batch's integer features) for tables of `dims` rows, cached on `holder` (the
    batch) per (field, tensor, dims) like the graph cache: one range check per batch, not one per call.  make: a map
    from the checked [R, K] codes to what is stored (ogbconv: the combined bond code)."""
    key = (field, tuple(int(d) for d in dims), make)
    stamp = tensor_stamp(codes)
    cache = None
    if holder is not None:
        cache = getattr(holder, "_mp_code_cache", None)
        if cache is None:
            cache = {}
            try:
                setattr(holder, "_mp_code_cache", cache)
            except Exception:
                cache = None
        if cache is not None:
            hit = cache.get(key)
            if hit is not None and hit[0] == stamp:
                return hit[2]
    out = ops.check_codes(codes, dims, what=field)
    if make is not None:
        out = make(out)
    if cache is not None:
        cache[key] = (stamp, codes, out)        # holding the tensor keeps its address unique
    return out


def _float_guard(t, what):
    if t.is_floating_point():
        raise TypeError("{} must hold integer codes, got {}".format(what, t.dtype))


class _TablesEncoder(nn.Module):
    """K embedding tables summed over the first K feature columns"""

    def _tables(self):
        raise NotImplementedError

    def encode(self, feature, holder, field, columns=None):
        tables = self._tables()
        _float_guard(feature, field)
        if feature.dim() == 1:
            feature = feature[:, None]
        K = min(feature.size(1), len(tables)) if columns is None else columns
        if feature.size(1) > len(tables) and columns is None:
            raise IndexError("{} has {} columns, the encoder has {} tables".format(field, feature.size(1), len(tables)))
        tables = tables[:K]
        dims = [t.size(0) for t in tables]
        codes = cached_codes(holder, field, feature[:, :K], dims)
        table = tables[0] if K == 1 else torch.cat(list(tables), dim=0)
        return ops.embed_sum(codes, table, table_offsets(dims))


class IntegerFeatureEncoder(_TablesEncoder):
    """feature_encoder.py:13-31"""

    def __init__(self, emb_dim, num_classes=None):
        super().__init__()
        self.encoder = nn.Embedding(num_classes, emb_dim)
        nn.init.xavier_uniform_(self.encoder.weight.data)

    def _tables(self):
        return [self.encoder.weight]

    def forward(self, batch):
        # Encode just the first dimension if more exist (feature_encoder.py:28-29)
        batch.node_feature = self.encode(batch.node_feature, batch, "node_feature", columns=1)
        return batch


class SingleAtomEncoder(_TablesEncoder):
    """feature_encoder.py:34-53"""

    def __init__(self, emb_dim, num_classes=None):
        super().__init__()
        self.atom_type_embedding = nn.Embedding(full_atom_feature_dims[0], emb_dim)
        nn.init.xavier_uniform_(self.atom_type_embedding.weight.data)

    def _tables(self):
        return [self.atom_type_embedding.weight]

    def forward(self, batch):
        batch.node_feature = self.encode(batch.node_feature, batch, "node_feature", columns=1)
        return batch


class AtomEncoder(_TablesEncoder):
    """feature_encoder.py:56-81"""

    def __init__(self, emb_dim, num_classes=None):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList()
        for dim in full_atom_feature_dims:
            emb = nn.Embedding(dim, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)

    def _tables(self):
        return [emb.weight for emb in self.atom_embedding_list]

    def forward(self, batch):
        batch.node_feature = self.encode(batch.node_feature, batch, "node_feature")
        return batch


class BondEncoder(_TablesEncoder):
    """feature_encoder.py:84-103"""

    def __init__(self, emb_dim):
        super().__init__()
        self.bond_embedding_list = nn.ModuleList()
        for dim in full_bond_feature_dims:
            emb = nn.Embedding(dim, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.bond_embedding_list.append(emb)

    def _tables(self):
        return [emb.weight for emb in self.bond_embedding_list]

    def forward(self, batch):
        batch.edge_feature = self.encode(batch.edge_feature, batch, "edge_feature")
        return batch


node_encoder_dict = {'Integer': IntegerFeatureEncoder, 'SingleAtom': SingleAtomEncoder, 'Atom': AtomEncoder}
edge_encoder_dict = {'Bond': BondEncoder}
