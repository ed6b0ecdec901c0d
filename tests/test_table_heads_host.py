"""Several heads over a neighbour table without a device: the exports, and the refusals of ops.knn_softmax(heads=),
ops.knn_aggr on a weight [.., H], KnnHypergraph.aggregate(heads=) and DynamicHypergraphConv(heads=) in their documented order -- dtype, then shapes, then gradients, then
the device -- on CPU tensors, so every case ends before a device is touched."""
import pytest
import torch

NEW = ("hg_table_softmax_heads_f32", "hg_table_softmax_bwd_heads_f32", "hg_table_sum_heads_f32", "hg_table_gather_heads_f32",
       "hg_table_gather_t_heads_f32", "hg_table_dot_heads_f32")
IDX = torch.zeros(6, 3, dtype=torch.int32)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    assert all(name in _lib.SYMBOLS and hasattr(L, name) for name in NEW) and L.hg_version() == 410


# every case carries a later refusal as well: the one named must come first
SOFTMAX = [
    (dict(node_score=z(9, 2, dtype=torch.bfloat16), heads=0), TypeError, "node_score must be a float32"),
    (dict(node_score=z(9, 2), group="nowhere", heads=0), ValueError, "group must be"),
    (dict(node_score=z(9), heads=0), ValueError, "heads must be an integer >= 1"),
    (dict(node_score=z(9), heads=True), ValueError, "heads must be an integer >= 1"),
    (dict(node_score=z(9), edge_score=z(5, 2), heads=2), ValueError, r"node_score must be \[n >= 1, heads = 2\]"),
    (dict(node_score=z(9, 3), edge_score=z(6, 2), heads=2), ValueError, r"node_score must be \[n >= 1, heads = 2\]"),
    (dict(node_score=z(9, 2), edge_score=z(6), heads=2), ValueError, r"edge_score must be \[rows, heads\] = \[6, 2\]"),
    (dict(node_score=z(9, 2), entry_score=z(6, 3), heads=2), ValueError, r"entry_score must be \[rows, k, heads\] = \[6, 3, 2\]"),
    (dict(node_score=z(9, 2), edge_score=z(6, 2), entry_score=z(18, 2), heads=2), RuntimeError, "idx must be on a GPU"),
]


@pytest.mark.parametrize("kw,error,text", SOFTMAX)
def test_knn_softmax_heads_refuses_in_order(hg, kw, error, text):
    with pytest.raises(error, match=text):
        hg.ops.knn_softmax(IDX, **kw)


# ops.knn_aggr takes the heads from the weight's last dimension: [rows * k, H] or [rows, k, H]
AGGR = [
    (dict(X=z(9, 8, dtype=torch.bfloat16), weight=z(18, 2), options="rows"), TypeError, "X must be a float32"),
    (dict(X=z(9, 7), weight=z(18, 2).double()), TypeError, "weight must be a float32"),
    (dict(X=z(9, 7), weight=z(18, 2), second="max"), ValueError, "take no weight"),
    (dict(X=z(9, 7), weight=z(18, 2), degE=z(5)), ValueError, "no multiple of heads = 2"),
    (dict(X=z(9, 7), weight=z(6, 3, 2)), ValueError, "no multiple of heads = 2"),
    (dict(X=z(9, 8), weight=z(17, 2)), ValueError, r"weight must be \[rows \* k\] = \[18\]"),
    (dict(X=z(9, 8), weight=z(6, 3, 2), degE=z(5)), ValueError, "degE must be"),
    (dict(X=z(9, 8), weight=z(6, 3, 2).requires_grad_(True)), RuntimeError, "weight gets no gradient"),
    (dict(X=z(9, 8), weight=z(6, 3, 2).requires_grad_(True), weight_grad=True), RuntimeError, "idx must be on a GPU"),
]


@pytest.mark.parametrize("kw,error,text", AGGR)
def test_knn_aggr_heads_refuses_in_order(hg, kw, error, text):
    kw = dict(kw)
    if kw.get("options") == "rows":
        kw["options"] = hg.ops.current_options().replace(incidence_bf16="rows")
    with pytest.raises(error, match=text):
        hg.ops.knn_aggr(IDX, kw.pop("X"), **kw)


@pytest.mark.parametrize("kw,text", [(dict(heads=0, weight=z(18, 2)), "heads must be an integer >= 1"),
                                     (dict(heads=2, weight=z(18)), "heads=2 needs weight"),
                                     (dict(heads=2), "heads=2 needs weight"),
                                     (dict(weight=z(6, 3, 2)), "heads=1 needs weight"),
                                     (dict(heads=2, weight=z(18, 2), probabilistic=True), "exclude each other")])
def test_aggregate_checks_heads_against_the_weight(hg, kw, text):
    g = hg.KnnHypergraph.__new__(hg.KnnHypergraph)
    g.idx = IDX
    with pytest.raises(ValueError, match=text):
        g.aggregate(z(6, 8), **kw)


@pytest.mark.parametrize("kw,text", [(dict(heads=0, attention="vertex"), "heads must be an integer >= 1"),
                                     (dict(heads=2.0, attention="vertex"), "heads must be an integer >= 1"),
                                     (dict(heads=2), "needs attention="),
                                     (dict(heads=2, attention="vertex", device_graph=False), "needs device_graph=True")])
def test_layer_heads_refusals(hg, kw, text):
    with pytest.raises(ValueError, match=text):
        hg.DynamicHypergraphConv(8, 4, k=3, **dict(dict(device_graph=True), **kw))


def test_layer_heads_parameters(hg):
    conv = hg.DynamicHypergraphConv
    torch.manual_seed(0)
    one = conv(8, 4, k=3, device_graph=True, attention="hyperedge")
    torch.manual_seed(0)
    same = conv(8, 4, k=3, device_graph=True, attention="hyperedge", heads=1, concat=False)
    assert all(torch.equal(a, b) for a, b in zip(one.state_dict().values(), same.state_dict().values()))
    layer = conv(8, 4, k=3, device_graph=True, attention="hyperedge", heads=3)
    assert sorted(layer.state_dict()) == ["a_e", "a_v", "lin.weight"]
    assert layer.a_v.shape == layer.a_e.shape == (12,) and layer.lin.weight.shape == (12, 8)
    assert float(layer.a_v.detach().abs().max()) <= (6.0 / 5) ** 0.5  # HypergraphAttnConv's bound: out_channels, not heads * out_channels
    with pytest.raises(TypeError, match="float32 rows"):
        layer.to(torch.bfloat16)(torch.zeros(9, 8, dtype=torch.bfloat16))
