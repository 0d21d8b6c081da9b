"""CPU: host-side logic — C-ABI exports, parameter/initialisation/checkpoint compatibility with the
reference (against the golden fixtures), string-dispatched configuration, collation, and loud
failure when no HIP device is behind the tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from glam_amd import _lib, layer, model, ops
from glam_amd.data import Batch, Data, DataLoader, synth_batch, synth_molecule, synth_protein_batch
from tests.conftest import ROOT, Golden, assert_close


def _header_source():
    src = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(glam_[a-z0-9_]+)\s*\(", _header_source())))


_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
              "size_t": ctypes.c_size_t}


def _header_prototypes():
    """name -> (return type, [parameter types]) of every prototype of include/glam_hip.h (they span lines up to ';'); a type is the
    ctypes scalar of _C_SCALARS, or "pointer" for anything with a '*'.  A type this does not know is a KeyError: extend the table."""
    def ctype(decl, named):
        words = [w for w in decl.split() if w != "const"]
        return "pointer" if "*" in decl else _C_SCALARS[" ".join(words[:-1] if named else words)]

    src = re.sub(r"^\s*#.*$", "", _header_source(), flags=re.M)
    return {name: (ctype(ret, False), [] if params.strip() == "void" else [ctype(q, True) for q in params.split(",")])
            for ret, name, params in re.findall(r"([\w \t*]+?)\b(glam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def _table_type(t):
    return "pointer" if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer) else t


def test_library_exports_every_declared_symbol():
    names = _header_functions()
    assert len(names) >= 16
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"libglam_hip.so does not export {n}"
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and include/glam_hip.h disagree"
    assert _lib.load().glam_abi_version() == _lib.ABI_VERSION == 4


def test_signature_table_has_the_types_of_the_header():
    """Names alone load fine with an int bound as int64_t, a float as double or an argument missing, and corrupt the call: every
    entry of SIGNATURES has the return type and, position by position, the parameter types of its prototype.  The header is the truth."""
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions()
    wrong = []
    for name, (res, args) in _lib.SIGNATURES.items():
        table = (_table_type(res), [_table_type(a) for a in args])
        if table != protos[name]:
            wrong.append(f"{name}: header {protos[name]}, table {table}")
    assert not wrong, "\n".join(wrong)


# the int-returning entry points whose int is a value, not a status: the checked view hands it through.  Adding one is an edit HERE too.
_UNCHECKED_INT = ["glam_abi_version", "glam_route_enabled", "glam_prof_end", "glam_ce_loss_max_classes", "glam_adam_max_tensors",
                  "glam_ranger_max_tensors", "glam_nnconv_ec_supported", "glam_pair_pool_add_supported", "glam_triplet_fwd_ell_supported",
                  "glam_triplet_layer_ws_supported", "glam_triplet_layer_infer_supported", "glam_relation_mlp_supported",
                  "glam_gru_fused_supported", "glam_gru_ws_supported", "glam_linear_narrow_supported", "glam_ts_gemm_relu_supported",
                  "glam_ts_gemm_rrelu_supported", "glam_graph_norm_drop_supported"]


def test_checked_view_checks_every_status_and_nothing_else():
    api, raw = _lib.api(), _lib.load()
    assert api is not raw and api is _lib.api()
    ints = [n for n, (res, _) in _lib.SIGNATURES.items() if res is ctypes.c_int]
    unchecked = sorted(n for n in ints if getattr(api, n).errcheck is None)
    assert unchecked == sorted(_UNCHECKED_INT) == sorted(_lib.VALUE_RETURNS)
    for n, (res, _) in _lib.SIGNATURES.items():
        assert getattr(raw, n).errcheck is None, f"load() must stay the raw binding ({n})"
        if res is not ctypes.c_int:
            assert getattr(api, n).errcheck is None, f"{n} returns a value"
        elif n not in _UNCHECKED_INT:
            assert getattr(api, n).errcheck is not None, f"{n} returns a status the checked view does not check"


def test_checked_view_raises_where_the_raw_binding_returns_a_code():
    api, raw = _lib.api(), _lib.load()
    bad_cp = (None, None, None, None, None, None, None, None, 10, 10, 3, 30, 4, 1, 0.2, None, None, None)
    with pytest.raises(_lib.GlamHipError) as e:
        api.glam_triplet_fwd(*bad_cp)
    assert "glam_triplet_fwd" in str(e.value) and "code -1" in str(e.value) and "multiple of 4" in str(e.value)
    assert str(e.value).startswith("glam_triplet_fwd failed (code -1): ")
    assert raw.glam_triplet_fwd(*bad_cp) == _lib.GLAM_E_INVALID
    with pytest.raises(_lib.GlamHipError, match="code -2"):
        api.glam_triplet_fwd(None, None, None, None, None, None, None, None, 10, 10, 3, 60, 5, 1, 0.2, None, None, None)


def test_checked_view_hands_values_through():
    api, raw = _lib.api(), _lib.load()
    assert api.glam_nnconv_ec_supported(4, 31, 60, 60) == 0 == raw.glam_nnconv_ec_supported(4, 31, 60, 60)     # (hidden = 32 only)
    assert raw.glam_nnconv_ec_supported(4, 32, 60, 60) == 1 == api.glam_nnconv_ec_supported(4, 32, 60, 60)
    assert api.glam_csr_workspace_bytes(1000, 3000) == raw.glam_csr_workspace_bytes(1000, 3000) > 0
    assert api.glam_abi_version() == raw.glam_abi_version() == _lib.ABI_VERSION
    assert api.glam_adam_max_tensors() == raw.glam_adam_max_tensors() > 0
    assert api.glam_last_error() == raw.glam_last_error()


def test_check_raises_on_a_non_zero_code_only():
    assert _lib.check(0, "x") is None
    with pytest.raises(_lib.GlamHipError, match=r"^x failed \(code -1\): "):
        _lib.check(-1, "x")


def test_abi_rejects_bad_arguments_without_touching_a_gpu():
    lib = _lib.load()
    # Cp not a multiple of 4 -> GLAM_E_INVALID before any launch
    rc = lib.glam_triplet_fwd(None, None, None, None, None, None, None, None, 10, 10, 3, 30, 4, 1, 0.2, None, None, None)
    assert rc == _lib.GLAM_E_INVALID and b"multiple of 4" in lib.glam_last_error()
    rc = lib.glam_triplet_fwd(None, None, None, None, None, None, None, None, 10, 10, 3, 60, 5, 1, 0.2, None, None, None)
    assert rc == _lib.GLAM_E_UNSUPPORTED
    # tensors beyond the 32-bit byte offsets of the aggregate kernels are refused, not silently wrapped
    rc = lib.glam_triplet_fwd(None, None, None, None, None, None, None, None, 6_000_000, 10, 3, 60, 4, 1, 0.2, None, None, None)
    assert rc == _lib.GLAM_E_UNSUPPORTED and b"4 GiB" in lib.glam_last_error()
    rc = lib.glam_pool5_fwd(None, None, 4, 2, 60, 9, None, None, None)
    assert rc == _lib.GLAM_E_UNSUPPORTED
    rc = lib.glam_csr_build(None, 4, 4, 2, None, None, None, None, None, 0, None)
    assert rc == _lib.GLAM_E_INVALID


def test_cpu_tensors_fail_loudly():
    conv = layer.TripletMessage(60, 4)
    b = synth_batch(2, seed=0)
    x = torch.randn(b.x.size(0), 60)
    with pytest.raises(_lib.GlamHipError, match="no CPU fallback"):
        conv(x, b.edge_index, b.edge_attr)
    with pytest.raises(_lib.GlamHipError):
        layer.GlobalPool5()(x, b.batch)
    with pytest.raises(_lib.GlamHipError):
        ops.GraphIndex(b.edge_index, x.size(0))


@pytest.mark.parametrize("name,C,De", [("triplet_c60", 60, 4), ("triplet_c15", 15, 4), ("triplet_de8", 60, 8)])
def test_triplet_init_matches_reference_under_seed(name, C, De):
    """Same parameter creation/initialisation order as layer.py:22-34 => identical weights from the
    same seed (oracle/gen_goldens.py seeds 11 + C + De before constructing the reference layer)."""
    g = Golden(name)
    torch.manual_seed(11 + C + De)
    conv = layer.TripletMessage(C, De)
    with torch.no_grad():
        conv.bias.normal_(0, 0.1)
    sd = conv.state_dict()
    assert list(sd) == ["weight_node", "weight_edge", "weight_triplet_att", "weight_scale", "bias"]
    for k, v in sd.items():
        assert torch.equal(v, g.params[k]), k


def test_light_init_matches_reference_under_seed():
    g = Golden("light_c60")
    torch.manual_seed(31 + 60)
    conv = layer.TripletMessageLight(60, 4)
    with torch.no_grad():
        conv.bias.normal_(0, 0.1)
    for k, v in conv.state_dict().items():
        assert torch.equal(v, g.params[k]), k


@pytest.mark.parametrize("name", ["arch_triplet_pool5", "arch_light_lapool"])
def test_architecture_state_dict_matches_reference(name):
    g = Golden(name)
    m = g.meta
    torch.manual_seed(62)
    np.random.seed(62)
    net = model.Architecture(e_dim=m["e_dim"], out_dim=m["out_dim"], message_steps=m["message_steps"],
                             mol_block=m["mol_block"], mol_readout=m["mol_readout"])
    sd = net.state_dict()
    assert list(sd) == list(g.params), "checkpoint keys / order differ from the reference"
    for k, v in sd.items():
        assert torch.equal(v, g.params[k]), f"{k}: init differs from the reference under the same seed"
    net.load_state_dict(g.params)   # reference checkpoints load unchanged


@pytest.mark.parametrize("name", ["block_triplet_relu", "block_triplet_pair_rrelu", "block_light_celu", "block_nnconv_relu",
                                  "block_gcn_relu", "block_gat_leaky"])
def test_message_block_state_dict_keys(name):
    g = Golden(name)
    m = g.meta
    blk = layer.MessageBlock(60, 60, 4, norm=m["norm"], dropout="_None()", conv=m["conv"], act=m["act"], res=True)
    assert [n for n, _ in blk.named_parameters()] == list(g.params)
    missing = blk.load_state_dict(g.params, strict=False)
    # the goldens store named_parameters(); PyG's GATConv registers the shared Linear twice (lin_l is lin_r)
    assert set(missing.missing_keys) <= {"conv.conv.lin_r.weight"} and not missing.unexpected_keys


def test_string_dispatch_surface():
    for conv in ["_TripletMessage", "_TripletMessageLight", "_NNConv", "_GCNConv", "_GATConv"]:
        blk = layer.MessageBlock(30, 30, 4, norm="_PairNorm", dropout="Dropout(0.1)", conv=conv, act="RReLU", res=1)
        assert (blk.gru is None) == (conv in ["_GCNConv", "_GATConv"])
    for norm in ["_None", "_BatchNorm", "_LayerNorm", "_PairNorm", "_GraphSizeNorm"]:
        for act in ["_None", "ReLU", "LeakyReLU", "RReLU", "CELU", "PReLU"]:
            layer.LinearBlock(8, 4, norm=norm, dropout="_None()", act=act)
    for ro in ["GlobalPool5", "GlobalLAPool", "Set2Set"]:
        net = model.Architecture(mol_block="_TripletMessage", mol_readout=ro, e_dim=32)
        assert net.mol_flat.linear.in_features == (300 if ro == "GlobalPool5" else 120)
    assert layer.TripletMessage(60, 4).extra_repr() == "60, 60, heads=3"
    import inspect
    for cls in (layer.TripletMessage, layer.TripletMessageLight):     # PyG lifts by these names (layer.py:42, :88)
        assert list(inspect.signature(cls.message).parameters)[1:] == ["x_j", "x_i", "edge_index_i", "edge_attr", "size_i"]
        assert list(inspect.signature(cls.update).parameters)[1:] == ["aggr_out"]
        assert callable(cls.propagate)


def test_collation_matches_pyg_semantics():
    rng = np.random.default_rng(3)
    mols = [synth_molecule(rng) for _ in range(5)]
    b = Batch.from_data_list(mols)
    off = 0
    e0 = 0
    for gidx, d in enumerate(mols):
        n, e = d.x.size(0), d.edge_index.size(1)
        assert torch.equal(b.x[off:off + n], d.x)
        assert torch.equal(b.edge_index[:, e0:e0 + e], d.edge_index + off)
        assert torch.equal(b.edge_attr[e0:e0 + e], d.edge_attr)
        assert (b.batch[off:off + n] == gidx).all()
        off += n
        e0 += e
    assert b.num_graphs == 5 and b.y.shape == (5, 1)
    assert (b.batch[1:] >= b.batch[:-1]).all()
    loader = DataLoader(mols, batch_size=2)
    assert len(loader) == 3 and [bb.num_graphs for bb in loader] == [2, 2, 1]


def test_synthetic_batches_have_the_reference_layout():
    b = synth_batch(64, seed=0)
    N, E = b.x.size(0), b.edge_index.size(1)
    assert b.x.shape == (N, 15) and b.edge_attr.shape == (E, 4) and b.edge_index.dtype == torch.int64
    assert 12 * 64 <= N <= 28 * 64 and 1.9 < E / N < 2.3
    src, dst = b.edge_index
    assert (b.batch[src] == b.batch[dst]).all(), "edges must not cross graphs"
    assert (src != dst).all()
    # symmetric: every (s,d) has its (d,s)
    fwd = set(zip(src.tolist(), dst.tolist()))
    assert all((d, s) in fwd for s, d in fwd)
    # per molecule sorted by src*n+dst (dataset.py:84-86) => globally sorted by (src, dst)
    key = src * N + dst
    assert (key[1:] > key[:-1]).all()
    assert torch.equal(b.edge_attr.sum(1), torch.ones(E)) and torch.equal(b.x[:, :9].sum(1), torch.ones(N))
    deg = torch.bincount(dst, minlength=N)
    assert deg.min() >= 1 and deg.max() <= 4
    p = synth_protein_batch(2, seed=1, n_min=50, n_max=80)
    assert p.x.size(1) == 49 and p.edge_attr.size(1) == 8


def test_model_args_filter():
    from types import SimpleNamespace
    args = SimpleNamespace(dataset="esol", seed=1, gpu=0, lr=1e-3, hid_dim_alpha=2, mol_block="_TripletMessage", e_dim=64)
    assert model.model_args(args) == {"hid_dim_alpha": 2, "mol_block": "_TripletMessage", "e_dim": 64}


def test_data_to_drops_device_caches():
    d = Data(torch.zeros(3, 2), torch.zeros(2, 0, dtype=torch.long))
    d._glam_cache = {"x": 1}
    assert not hasattr(d.to("cpu"), "_glam_cache")


def test_flat_view_recognises_bucket_views():
    from glam_amd.parallel import flat_view
    buf = torch.arange(20, dtype=torch.float32)
    a, b, c = (t.view(s) for t, s in zip(buf[2:].split([6, 4, 8]), ((2, 3), (4,), (2, 4))))
    fv = flat_view([a, b, c])
    assert fv is not None and fv.data_ptr() == a.data_ptr() and fv.numel() == 18
    fv.mul_(2)
    assert float(c[1, 3]) == 38.0                       # reductions on the bucket show through the gradients
    assert flat_view([a, c]) is None                    # gap
    assert flat_view([a, torch.zeros(4)]) is None       # different storage
    assert flat_view([]) is None


def test_dataloader_caches_collated_batches_when_order_is_fixed():
    rng = np.random.default_rng(5)
    mols = [synth_molecule(rng) for _ in range(7)]
    loader = DataLoader(mols, batch_size=3)                  # shuffle=False => cached
    first = list(loader)
    second = list(loader)
    assert len(first) == 3 and all(a is b for a, b in zip(first, second))       # same objects: CSR cache keys stay valid
    assert all(a.edge_index is b.edge_index for a, b in zip(first, second))
    fresh = list(DataLoader(mols, batch_size=3, cache=False))
    assert all(torch.equal(a.x, b.x) and torch.equal(a.edge_index, b.edge_index) for a, b in zip(first, fresh))
    shuffled = DataLoader(mols, batch_size=3, shuffle=True, seed=1)
    assert [b.num_graphs for b in shuffled] == [3, 3, 1] and shuffled.cache is False
    with pytest.raises(ValueError):
        DataLoader(mols, batch_size=3, shuffle=True, cache=True)


def test_gpu_manager_surface(monkeypatch):
    """Search-loop device picker (utils.py:185-246) without nvidia-smi: same keys and choices, fed by the HIP runtime."""
    from glam_amd.devices import GPUManager
    if not torch.cuda.is_available():
        m = GPUManager()
        assert m.gpu_num == 0 and m.auto_choice(0.5) is None and m.wait_free_gpu() == -1
    mem = {0: (10 << 30, 288 << 30), 1: (250 << 30, 288 << 30), 2: (200 << 30, 288 << 30)}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 3)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda i: mem[i])
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda i: "AMD Instinct MI355X")
    m = GPUManager(["power.draw"])
    assert m.gpu_num == 3 and set(m.gpus[0]) == {"index", "gpu_name", "memory.free", "memory.total", "power.draw"}
    assert m.gpus[1]["memory.free"] == 250 * 1024 and m.auto_choice(0.7) == 1 and m.wait_free_gpu(0.7) == 1
    mem[1] = (100 << 30, 288 << 30)
    assert m.auto_choice(0.7) is None and m.auto_choice(0.5) == 2


def test_packed_dataset_collates_like_from_data_list():
    """Vectorised collation (flat dataset + gathers) == PyG-style concatenation, for contiguous and shuffled graph ids,
    single-row and multi-row labels, graphs without edges; the DataLoader uses it for every batch."""
    import numpy as np
    from glam_amd.data import Batch, Data, DataLoader, PackedDataset, synth_molecule
    rng = np.random.default_rng(3)
    mols = [synth_molecule(rng) for _ in range(40)]
    mols[7] = Data(mols[7].x[:1], torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 4), y=mols[7].y)     # single atom, no bonds
    pk = PackedDataset(mols)
    for ids in (np.arange(0, 16), np.arange(30, 40), rng.permutation(40)[:13], np.array([7]), np.array([], dtype=np.int64)):
        a = Batch.from_data_list([mols[i] for i in ids]) if len(ids) else None
        b = pk.collate(ids)
        if a is None:
            assert b.x.size(0) == 0 and b.edge_index.size(1) == 0 and b.num_graphs == 0
            continue
        for k in ("x", "edge_index", "edge_attr", "y", "batch", "ptr"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert a.num_graphs == b.num_graphs
    for m in mols:                                              # two label rows per graph
        m.y = torch.randn(2, 3)
    pk2 = PackedDataset(mols)
    ids = rng.permutation(40)[:9]
    assert torch.equal(pk2.collate(ids).y, Batch.from_data_list([mols[i] for i in ids]).y)
    got = [b.x.size(0) for b in DataLoader(mols, batch_size=16, shuffle=True, seed=5)]
    assert sum(got) == sum(m.x.size(0) for m in mols) and len(got) == 3


def test_loader_batches_carry_host_side_validation_marks():
    """PackedDataset validates ids / one-hot rows once on the host; the marks ride on the collated tensors (and survive
    ``.to()``), so the device-side staging reads nothing back for loader-built batches."""
    import numpy as np
    from glam_amd.data import DataLoader, PackedDataset, synth_molecule
    rng = np.random.default_rng(1)
    mols = [synth_molecule(rng) for _ in range(10)]
    b = next(iter(DataLoader(mols, batch_size=4, shuffle=True, seed=2)))
    b2 = b.to("cpu")
    for t in (b.edge_index, b.batch, b2.edge_index, b2.batch):
        assert getattr(t, "_glam_trusted", None) == t._version
    assert b2.edge_attr._glam_onehot == (True, b2.edge_attr._version)
    b2.edge_index[0, 0] = 0                                            # an in-place write voids the mark
    assert b2.edge_index._glam_trusted != b2.edge_index._version
    mols[3].edge_attr = mols[3].edge_attr * 0.5                       # not one-hot any more
    assert PackedDataset(mols).collate(np.arange(4)).edge_attr._glam_onehot[0] is False
    mols[5].edge_index = mols[5].edge_index.clone()
    mols[5].edge_index[0, 0] = 99                                      # an id outside its graph: no trust mark, the device checks
    bad = PackedDataset(mols).collate(np.arange(4, 8))
    assert getattr(bad.edge_index, "_glam_trusted", None) is None


def test_validation_marks_do_not_survive_a_write_or_a_replacement_across_to():
    """``Data.to()`` copies the mark of the very tensor it moves, and only while that mark is valid: a tensor written in
    place after collation, or a different tensor assigned to the field, arrives on the device unmarked (so the device-side
    staging validates it: R-GCN one-hot path not taken on scaled features, bad ids raise IndexError)."""
    import numpy as np
    from glam_amd.data import PackedDataset, synth_molecule
    rng = np.random.default_rng(4)
    mols = [synth_molecule(rng) for _ in range(6)]
    pk = PackedDataset(mols)
    meta = torch.device("meta")                                        # a real copy (new tensor objects) without a GPU

    b = pk.collate(np.arange(6))
    ok = b.to(meta)
    assert ok.edge_index._glam_trusted == ok.edge_index._version and ok.batch._glam_trusted == ok.batch._version
    assert ok.edge_attr._glam_onehot == (True, ok.edge_attr._version)

    b = pk.collate(np.arange(6))
    b.edge_attr.mul_(0.5)                                              # write, then to(): no one-hot mark on the copy
    moved = b.to(meta)
    assert getattr(moved.edge_attr, "_glam_onehot", None) is None
    assert moved.edge_index._glam_trusted == moved.edge_index._version   # untouched fields keep theirs

    b = pk.collate(np.arange(6))
    b.edge_index = torch.full((2, 3), 10 ** 6)                         # replace, then to(): the new tensor was never validated
    b.batch = b.batch.clone()
    moved = b.to(meta)
    assert getattr(moved.edge_index, "_glam_trusted", None) is None
    assert getattr(moved.batch, "_glam_trusted", None) is None


def test_torch_extension_registers_the_boundary_ops_and_refuses_cpu_tensors():
    """the hot path is exposed through a torch extension (TORCH_LIBRARY(glam)): every operator of the list is
    registered with torch's dispatcher from the in-tree _glam_torch.so, and a CPU tensor is a RuntimeError (TORCH_CHECK), never a
    silent CPU computation."""
    from glam_amd import torch_ext
    ns = torch_ext.load()
    for name in torch_ext.OPS:
        assert hasattr(ns, name), name
    sch = str(ns.triplet_layer.default._schema)
    assert "weight_triplet_att" in sch and "int heads" in sch
    with pytest.raises(RuntimeError, match="HIP device only"):
        ns.csr_from_edge_index(torch.zeros(2, 3, dtype=torch.long), 4, 0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ns.segment_pool(torch.zeros(4, 8), torch.zeros(3, dtype=torch.int32), 0)


def test_adam_restatement_matches_the_library_optimizer_on_cpu():
    """The arithmetic of ``csrc/optim.hip`` (``oracle.adam_step``: fp32, bias corrections as -expm1(s ln beta)) against
    ``torch.optim.Adam`` — the optimizer the reference's trainer constructs (trainer.py:49-50) — over 60 steps with a learning-rate
    change and weight decay: 2e-6 of the largest parameter, moments to 1e-6.  The GPU test compares the kernel with the same reference."""
    from oracle import glam_oracle as oracle
    rng = np.random.default_rng(5)
    for wd in (0.0, 1e-2):
        p0 = rng.standard_normal(257).astype(np.float32)
        tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.Adam([tp], lr=1e-2, weight_decay=wd)
        p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        lr = 1e-2
        for step in range(60):
            if step == 20:
                lr = opt.param_groups[0]["lr"] = 3e-3
            g = (rng.standard_normal(257) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)
            tp.grad = torch.from_numpy(g.copy())
            opt.step()
            p, m, v = oracle.adam_step(p, g, m, v, step, lr=lr, weight_decay=wd)
        scale = max(1.0, float(np.abs(p).max()))
        assert np.abs(p - tp.detach().numpy()).max() <= 2e-6 * scale
        st = opt.state[tp]
        assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-6 * max(1.0, float(np.abs(m).max()))
        assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-6 * max(1.0, float(np.abs(v).max()))


def test_adam_abi_rejects_bad_arguments_without_touching_a_gpu():
    import ctypes
    lib = _lib.load()
    assert lib.glam_adam_max_tensors() >= 36          # a default-shaped model's parameter list goes in one launch
    tab = (ctypes.c_uint64 * 4)(0, 0, 0, 0)
    numel = (ctypes.c_int64 * 1)(8)
    args = (0.001, 0.9, 0.999, 1e-8, 0.0, None)
    assert lib.glam_adam_step(tab, numel, 1, None, None, None, *args) == _lib.GLAM_E_INVALID            # no step counter / ticket
    assert lib.glam_adam_step(tab, numel, 1, 8, 8, None, *args) == _lib.GLAM_E_INVALID                  # null tensor addresses
    assert lib.glam_adam_step(tab, numel, 1, 8, 8, None, 0.001, 1.0, 0.999, 1e-8, 0.0, None) == _lib.GLAM_E_INVALID   # beta1 = 1
    assert lib.glam_adam_step(tab, numel, 0, 8, 8, None, *args) == 0                                    # nothing to do


def test_padded_view_registry_is_host_logic():
    """ops.slice_cols / pad_cols / padded_base (the zero-padded flow of the odd hidden widths): pure bookkeeping, no kernels.  A view
    finds its padded tensor by address, strides and version; a view of a VIEW keeps the registered object alive; an in-place write or a
    different stride ends the trust."""
    import gc
    xp = torch.zeros(6, 48)
    xp[:, :45] = torch.randn(6, 45)
    v = ops.slice_cols(xp, 45)
    assert v.shape == (6, 45) and ops.padded_base(v) is xp and ops.pad_cols(v, 48) is xp
    assert ops.padded_base(v.unsqueeze(0).squeeze(0)) is xp                 # any view with the same address and strides
    assert ops.padded_base(xp) is None and ops.slice_cols(xp, 48) is xp     # nothing to slice
    # a registered tensor that is itself a view (the skip-connection alias of the layer node): its slice keeps it alive
    alias = xp.view_as(xp)
    w = ops.slice_cols(alias, 45)
    del alias
    gc.collect()
    assert ops.padded_base(w) is not None and ops.padded_base(w).data_ptr() == xp.data_ptr()
    w.add_(1.0)                                                             # the pad columns may no longer be what the producer left
    assert ops.padded_base(w) is None
    p = ops.pad_cols(w, 48)
    assert p.shape == (6, 48) and torch.equal(p[:, :45], w) and (p[:, 45:] == 0).all()
    other = torch.zeros(6, 52)[:, :45]                                      # a view nobody registered, another pitch
    assert ops.padded_base(other) is None


def test_pad_group_and_new_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks of the entry points added in round 4 run before any device work."""
    import ctypes
    lib = _lib.load()
    one = (ctypes.c_void_p * 1)(1 << 20)
    assert lib.glam_pad_group(9, one, one, (ctypes.c_int32 * 45)(), 0, None) == _lib.GLAM_E_INVALID
    assert lib.glam_pad_group(1, one, one, (ctypes.c_int32 * 5)(1, 4, 4, 3, 4), 0, None) == _lib.GLAM_E_INVALID     # padded < plain
    assert lib.glam_pad_group(0, None, None, None, 0, None) == 0
    assert lib.glam_gru_ws_supported(60) == 1 and lib.glam_gru_ws_supported(20) == 0 and lib.glam_gru_ws_supported(62) == 0
    assert lib.glam_gru_ws_fwd(None, None, None, None, None, None, None, 4, 20, 0, 1, 0.0, None, None, None, None, None) == _lib.GLAM_E_UNSUPPORTED
    assert lib.glam_gru_bwd_ws(None, None, None, None, None, None, None, None, None, 4, 62, 0, 1, 0.0, 0, None, None, None, None, None, None) == _lib.GLAM_E_UNSUPPORTED
    assert lib.glam_pool5_padded_fwd(None, None, 4, 2, 50, 45, 3, None, None, None) == _lib.GLAM_E_INVALID             # ld is not ceil4(D)
    assert lib.glam_ts_gemm_image_bytes(276, 92) > 0 and lib.glam_ts_gemm_image_bytes(300, 92) >= 0


def test_dense_gemm_entry_points_reject_bad_arguments_without_a_gpu():
    """glam_dense_gemm / glam_linear_dense_fwd / _bwd check strides, sizes and the all-ones column's layout before any launch."""
    lib = _lib.load()
    p = 1 << 20
    inv = _lib.GLAM_E_INVALID
    assert lib.glam_dense_gemm(p, 300, 2, None, 0.0, p, 1, 300, None, 0, 0.0, p, 64, None, 8, 64, 300, None) == inv      # no unit stride in A
    assert b"A's strides" in lib.glam_last_error()
    assert lib.glam_dense_gemm(p, 300, 1, None, 0.0, p, 3, 300, None, 0, 0.0, p, 64, None, 8, 64, 300, None) == inv      # ... nor in B
    assert lib.glam_dense_gemm(p, 300, 1, None, 0.0, p, 1, 300, None, 0, 0.0, p, 64, p, 8, 64, 300, None) == inv         # ones column, B along k
    assert lib.glam_dense_gemm(p, 300, 1, None, 0.0, p, 1, 300, None, 3, 0.0, p, 64, None, 8, 64, 300, None) == inv      # unknown activation
    assert lib.glam_dense_gemm(p, 300, 1, None, 0.0, p, 1, 300, None, 0, 0.0, p, 60, None, 8, 64, 300, None) == inv      # ldc < Cn
    assert lib.glam_dense_gemm(p, 2, 1, None, 0.0, p, 1, 2, None, 0, 0.0, p, 64, None, 8, 64, 2, None) == inv            # K < 4
    assert lib.glam_dense_gemm(None, 300, 1, None, 0.0, p, 1, 300, None, 0, 0.0, p, 64, None, 8, 64, 300, None) == inv   # null operand
    assert lib.glam_linear_dense_fwd(p, p, None, 0, 300, 64, 0, 0.0, p, None) == inv
    assert lib.glam_linear_dense_bwd(p, p, p, None, 0.0, 2, 300, 64, p, p, None, None) == inv                            # N < 4
    assert lib.glam_linear_dense_bwd(p, p, p, None, 0.0, 8, 300, 64, None, None, None, None) == inv                      # nothing to compute
    assert lib.glam_linear_dense_bwd(p, p, p, None, 0.0, 8, 300, 64, p, None, p, None) == inv                            # db without dw
    assert ops.linear_dense_supported(1024, 300, 1024) and not ops.linear_dense_supported(1024, 450, 1024) and not ops.linear_dense_supported(64, 1024, 617)
    assert not ops.linear_dense_supported(2, 300, 1024) and not ops.linear_dense_supported(1024, 16, 1024)
    assert lib.glam_prestage(None, None, None, None, None, 0, 0, 0, 0, 0, None, 0, None, None, None, None) == inv          # nothing to build
    assert lib.glam_prestage(None, None, None, None, None, 0, 0, 0, 0, 0, None, 7, None, None, None, None) == inv          # more than six images


def test_launch_saving_hints_are_host_logic():
    """following_dropout (the hint that lets an activation launch write the dropped twin), the prestage item lists and the operand-set
    thresholds are decided on the host: a training-mode Dropout with nothing in front of it gives its p, anything else 0; CPU tensors
    stage nothing."""
    blk = layer.LinearBlock(1024, 1, norm="_None", dropout="Dropout(0.2)", act="_None")
    assert layer.following_dropout(blk.train()) == pytest.approx(0.2)
    assert layer.following_dropout(blk.eval()) == 0.0
    assert layer.following_dropout(layer.LinearBlock(60, 60, norm="_PairNorm", dropout="Dropout(0.2)").train()) == 0.0     # a norm sits in front
    assert layer.following_dropout(layer.LinearBlock(60, 60, norm="_None", dropout="_None()").train()) == 0.0
    mb = layer.MessageBlock(60, 60, 4, norm="_None", dropout="Dropout(0.1)", conv="_TripletMessage", act="RReLU()").train()
    assert layer.following_dropout(mb) == pytest.approx(0.1)
    lin = layer.LinearBlock(15, 60)
    x, ea = torch.randn(40, 15), torch.zeros(80, 4)
    assert layer.prestage_pass((lin, mb, x, ea)) == 0                 # CPU tensors: nothing to stage, nothing launched
    trip, images, pres = layer._prestage_items(lin, mb, x.to("meta") if False else x, ea)
    assert trip is None and images == [] and pres == []
    assert ops.prestage(None, []) == 0 and ops.prestage(None, [], [(torch.zeros(180, 60), torch.zeros(180, 60), 60)]) == 0      # no scope: nothing built
    # ops.cat_cols outside its class (CPU tensors, no gradient wanted, more than eight pieces) is torch.cat
    a, b = torch.randn(3, 2, requires_grad=True), torch.randn(3, 4)
    assert torch.equal(ops.cat_cols([a, b]), torch.cat([a, b], dim=-1)) and not type(ops.cat_cols([a, b]).grad_fn).__name__.startswith("_CatCols")
    assert ops.cat_cols([torch.zeros(2, 1)] * 9).shape == (2, 9)
    assert ops.GRU_WGRAD_BATCH in (True, False) and ops.PRESTAGE in (True, False) and ops.NORM_DROP in (True, False) and ops.DENSE_LINEAR in (True, False)



def test_gradient_carry_threads_one_flat_buffer_through_a_blocks_applications(monkeypatch):
    """ops._Carry on CPU tensors: the block's first application of a pass is told apart from the later ones (three and four
    applications), every application gets the carry the previous one stored, and the bundle's backward hands each parameter the view
    of its piece of the flat buffer — consecutive pieces, in parameter order unless ``order`` says otherwise."""
    w, b = torch.randn(3, 4, requires_grad=True), torch.randn(3, requires_grad=True)
    for n in (3, 4):
        with ops.weight_scope():
            firsts, carries = [], []
            for _ in range(n):
                c = ops._Carry(("carry-test", id(w)), (w, b), ((3, 4), (3,)))
                assert c.tensor is not None and (not carries or c.tensor is carries[-1])
                firsts.append(c.first)
                carries.append(c.tensor.view(-1))       # (what a node returns as its carry output)
                c.store(carries[-1])
        assert firsts == [True] + [False] * (n - 1)
    g = torch.arange(15.0)
    dw, db = torch.autograd.grad(carries[0], (w, b), g)
    assert torch.equal(dw, g[:12].view(3, 4)) and torch.equal(db, g[12:])
    assert dw.data_ptr() == g.data_ptr() and db.data_ptr() == g.data_ptr() + 12 * 4       # views, no copies
    views = ops._flat_views(g, ((3, 4), (3,)))
    assert [v.shape for v in views] == [(3, 4), (3,)] and views[1].data_ptr() == views[0].data_ptr() + views[0].numel() * 4
    # memory order != parameter order (the GRU's [d_w_ih | d_b_ih | d_w_hh | d_b_hh] for (w_ih, w_hh, b_ih, b_hh))
    w2, b2 = torch.randn(3, 4, requires_grad=True), torch.randn(3, requires_grad=True)
    with ops.weight_scope():
        c = ops._Carry(("carry-test", id(w)), (w, w2, b, b2), ((3, 4), (3,), (3, 4), (3,)), order=(0, 2, 1, 3))
    g = torch.arange(30.0)
    gw, gw2, gb, gb2 = torch.autograd.grad(c.tensor, (w, w2, b, b2), g)
    assert torch.equal(gw, g[:12].view(3, 4)) and torch.equal(gb, g[12:15]) and torch.equal(gw2, g[15:27].view(3, 4)) and torch.equal(gb2, g[27:])
    # no carry outside a scope, without gradients, or with the switch off
    assert ops._Carry(("carry-test", id(w)), (w, b), ((3, 4), (3,))).tensor is None
    with ops.weight_scope():
        with torch.no_grad():
            assert ops._Carry(("carry-test", id(w)), (w, b), ((3, 4), (3,))).tensor is None
        monkeypatch.setattr(ops, "GRAD_CARRY", False)
        assert ops._Carry(("carry-test", id(w)), (w, b), ((3, 4), (3,))).tensor is None
    flat, d = torch.ones(4), torch.full((4,), 2.0)
    assert ops._carried(flat, None) is flat and torch.equal(ops._carried(flat, d, summed=True), torch.ones(4))
    assert ops._carried(flat, d) is flat and torch.equal(flat, torch.full((4,), 3.0))


def test_parked_weight_gradient_sets_are_launched_by_the_first_application(monkeypatch):
    """ops._park with fake launches: the later applications park (their backward runs first), the first one gets every parked set in
    groups of at most three that never mix compatibility keys and keep parking order, and the parked list is empty after a flush even
    when a launch raises (a retried backward must not count a set twice)."""
    scope, owner = ops._WeightScope(), torch.zeros(1)

    def flush(first_set, compat=None):
        launched = []
        addend = None
        for grp in ops._park(scope, "test", owner, True, first_set, compat):
            launched.append((list(grp), addend))         # (a launch chains the previous group's result in as its addend)
            addend = len(launched)
        return launched

    for n in (3, 4):                                     # applications n, ..., 2 park; application 1 launches
        assert all(ops._park(scope, "test", owner, False, k) is None for k in range(n, 1, -1))
        assert flush(1) == ([([3, 2, 1], None)] if n == 3 else [([4, 3, 2], None), ([1], 1)])
    keys = "abaaba"
    for k in range(5):
        ops._park(scope, "test", owner, False, k, keys[k])
    assert flush(5, keys[5]) == [([0, 2, 3], None), ([1, 4], 1), ([5], 2)]
    ops._park(scope, "test", owner, False, "later")

    def failing_launch(grp):
        raise RuntimeError("launch failed")
    with pytest.raises(RuntimeError):
        for grp in ops._park(scope, "test", owner, True, "first"):
            failing_launch(grp)
    assert ops._park(scope, "test", owner, True, None) == []
    assert ops._parks(scope, 512) and not ops._parks(scope, 511) and not ops._parks(None, 4096)
    monkeypatch.setattr(ops, "GRU_WGRAD_BATCH", False)
    assert not ops._parks(scope, 4096)


@pytest.mark.parametrize("kind", ["id", "ptr"])
def test_tensor_memo_entries_follow_the_tensors_life_and_version(kind):
    """glam_amd._memo.TensorMemo on CPU tensors: an entry goes when its tensor dies, misses after an in-place write until registered
    again, ``take`` pops, another tensor object over the same rows hits only a "ptr" table asked with ``same_object=False``, and an
    object that takes no weak references is not stored."""
    import gc
    from glam_amd._memo import TensorMemo
    memo = TensorMemo(kind)
    t = torch.zeros(4, 6)
    memo.put(t, "a")
    assert len(memo) == 1 and memo.get(t) == "a" and memo.referent(t) is t
    t.add_(1)
    assert memo.get(t) is None and memo.take(t) is None and memo.referent(t) is None and len(memo) == 1
    memo.put(t, "b")
    assert memo.get(t) == "b"
    twin = t.detach()                                    # another object, the same rows, the same version counter
    assert memo.get(twin) is None and memo.take(twin) is None
    assert memo.get(twin, same_object=False) == ("b" if kind == "ptr" else None)
    assert memo.referent(twin) is (t if kind == "ptr" else None)
    assert memo.take(t) == "b" and memo.take(t) is None and len(memo) == 0
    memo.put(t, "c")
    del t, twin
    gc.collect()
    assert len(memo) == 0
    memo.put(torch.zeros(2), 1)
    memo.clear()
    assert len(memo) == 0

    class Plain:                                         # (no __weakref__ slot)
        __slots__ = ("_version",)

        def data_ptr(self):
            return 64
    obj = Plain()
    obj._version = 0
    memo.put(obj, "x")
    assert len(memo) == 0 and memo.get(obj) is None


@pytest.mark.parametrize("kind", ["id", "ptr"])
def test_tensor_memo_finaliser_spares_a_newer_entry_under_the_same_key(kind):
    """Ids and addresses come back.  Tensor B registered under the key tensor A still holds: when A dies, its finaliser must leave B's
    entry alone.  Replacing an entry drops its weakref, and a dead weakref calls nothing, so A's finaliser only runs at all while
    something else still holds A's entry: the test holds it."""
    import gc
    from glam_amd._memo import TensorMemo
    memo = TensorMemo(kind)
    a = torch.zeros(4, 6)
    b = a.detach()                                       # shares a's data_ptr and keeps the storage, not a, alive
    if kind == "id":
        memo._key = lambda t: 7                          # two live objects never share an id: force the slot
    memo.put(a, "a")
    held = list(memo._d.values())                        # A's entry, and with it A's weakref, outlives its place in the table
    memo.put(b, "b")
    del a
    gc.collect()
    assert held[0][0]() is None and len(memo) == 1 and memo.get(b) == "b"
    del b
    gc.collect()
    assert len(memo) == 0


def test_tensor_side_tables_of_ops_keep_their_hit_conditions(monkeypatch):
    """The tables of glam_amd.ops behind TensorMemo, on CPU tensors (pure bookkeeping): the padded-view registry does not pop and ends
    with a write to the base; a dropped twin goes to the very tensor it was registered for with the very ``p``, once; a node product
    goes to any tensor object over the registered rows with the same shape and the same staged images, once."""
    xp = torch.zeros(6, 48)
    v = ops.slice_cols(xp, 45)
    assert ops.padded_base(v) is xp and ops.padded_base(v) is xp
    xp.add_(1.0)
    assert ops.padded_base(v) is None

    out, twin = torch.randn(5, 8), torch.randn(5, 8)
    ops.register_dropped(out, twin, 0.2)
    assert ops.take_dropped(out, 0.1) is None                       # another rate: no hit, and the entry stays
    assert ops.take_dropped(out.detach(), 0.2) is None              # another tensor object
    assert ops.take_dropped(out, 0.2) is twin and ops.take_dropped(out, 0.2) is None
    ops.register_dropped(out, twin, 0.2)
    out.mul_(2.0)
    assert ops.take_dropped(out, 0.2) is None

    monkeypatch.setattr(ops, "NODE_IN_GRU", True)
    rows, staged, xw, a_ij = torch.randn(16, 24), object(), torch.randn(16, 96), torch.randn(16, 8)
    ops.register_node_product(rows, staged, xw, a_ij)
    assert ops.take_node_product(rows, object()) is None            # other staged images
    assert ops.take_node_product(rows.view(8, 48), staged) is None  # another shape over the same address
    assert ops.take_node_product(rows.as_strided((16, 24), (1, 16)), staged) is None      # the same shape, not contiguous
    got = ops.take_node_product(rows.detach(), staged)              # another tensor object over the same rows: a hit
    assert got is not None and got[0] is xw and got[1] is a_ij
    assert ops.take_node_product(rows, staged) is None              # taken
    ops.register_node_product(rows, staged, xw, a_ij)
    monkeypatch.setattr(ops, "NODE_IN_GRU", False)
    assert ops.take_node_product(rows, staged) is None
    monkeypatch.setattr(ops, "NODE_IN_GRU", True)
    rows.add_(1.0)
    assert ops.take_node_product(rows, staged) is None


def test_weight_scope_interface_and_entry_constructors():
    """ops._WeightScope on CPU tensors with a fake ``build_fn``: ``lookup`` misses when another object sits under the key (a reused
    ``id()``: what the owner pin is for), ``build`` builds once per (table, key, owner) and every time without a scope, the two tables
    are separate, ``weight_scope()`` clears "fwd" on exit and keeps "bwd"; every key / image constructor gives equal keys for the same
    tensors and different keys for different ones."""
    calls = []

    def build_fn():
        calls.append(1)
        return len(calls)

    a, b = torch.zeros(2), torch.zeros(2)
    scope = ops._WeightScope()
    assert scope.lookup("fwd", ("k", 7), a) is None
    scope.store("fwd", ("k", 7), a, "va")
    assert scope.lookup("fwd", ("k", 7), a) == "va" and scope.lookup("fwd", ("k", 7), b) is None      # same key, another owner
    assert scope.lookup("bwd", ("k", 7), a) is None                                                   # separate tables
    assert scope.build("fwd", ("n", 1), a, build_fn) == 1 and scope.build("fwd", ("n", 1), a, build_fn) == 1 and len(calls) == 1
    assert scope.build("bwd", ("n", 1), a, build_fn) == 2 and scope.build("fwd", ("n", 2), a, build_fn) == 3
    assert scope.build("fwd", ("n", 1), b, build_fn) == 4 and scope.lookup("fwd", ("n", 1), a) is None       # the new owner took the slot
    assert ops.scope_build(scope, "bwd", ("n", 1), a, build_fn) == 2 and len(calls) == 4
    assert ops.scope_build(None, "fwd", ("n", 1), a, build_fn) == 5 and ops.scope_build(None, "fwd", ("n", 1), a, build_fn) == 6
    assert ops.scoped_weights(("n", 1), a, build_fn) == 7 and ops.scoped_weights(("n", 1), a, build_fn) == 8      # no active scope
    with ops.weight_scope():
        inner = ops._SCOPE
        assert ops.scoped_weights(("n", 1), a, build_fn) == 9 and ops.scoped_weights(("n", 1), a, build_fn) == 9
        inner.store("bwd", ("t", 1), a, "kept")
        assert inner.lookup("fwd", ("n", 1), a) == 9
    assert ops._SCOPE is None and inner.lookup("fwd", ("n", 1), a) is None and inner.lookup("bwd", ("t", 1), a) == "kept"

    t = [torch.zeros(8, 4) for _ in range(6)]
    keys = []
    for make, n in ((ops.triplet_key, 5), (lambda *ts: ops.triplet_key(*ts, plain=True), 5), (ops.triplet_ell_key, 1), (ops.gru_pre_key, 2),
                    (ops.gru_fused_key, 2), (ops.gru_pad_key, 4), (lambda w: ops.lin_image(w)[:2], 1), (lambda w: ops.lin_dx_image(w)[:2], 1),
                    (lambda w: ops.tall_image(w)[:2], 1), (lambda w: ops.tall_dx_image(w)[:2], 1)) + \
            tuple((lambda w, k=k: k(w, W=t[5])[:2], 1) for k in (ops.wide_node_image, ops.wide_upd_image, ops.wide_dagg_image, ops.wide_dx_image)):
        assert make(*t[:n]) == make(*t[:n])
        for i in range(n):          # any one tensor replaced: another key
            assert make(*(t[:i] + [t[n]] + t[i + 1:n])) != make(*t[:n])
        keys.append(make(*t[:n]))
    assert len(set(keys)) == len(keys)       # no two kinds share a (table, key) for the same tensors


def test_image_specs_reproduce_the_tuples_the_ops_and_the_prestage_lists_were_written_with():
    """The ``ImageSpec`` constructors against the 9-tuples ``(table, key, owner, W, ldw, transW, K, M, K_image)`` written out by hand for
    the shapes in use: the input linear 15 -> 60 on 16 zero-padded columns, the GRU's gate matrices at C = 60, the four images of
    the wide layer at H = 3, Cp = 92."""
    def same(spec, want):
        return len(spec) == len(want) == 9 and all((a is b) if isinstance(b, torch.Tensor) else (a == b and type(a) is type(b))
                                                   for a, b in zip(spec, want))

    w = torch.zeros(60, 15)
    assert same(ops.lin_image(w, 16), ("fwd", ("lin", id(w)), w, w, 15, 1, 15, 60, 16))
    g = torch.zeros(180, 60)
    assert same(ops.lin_image(g), ("fwd", ("lin", id(g)), g, g, 60, 1, 60, 180, 60))
    assert same(ops.lin_dx_image(g), ("bwd", ("lin", id(g)), g, g, 60, 0, 180, 60, 180))
    r = torch.zeros(300, 60)              # NNConv's relation product, stored [K, M]
    assert same(ops.tall_image(r), ("fwd", ("tall-fwd", id(r)), r, r, 60, 0, 300, 60, 300))
    assert same(ops.tall_dx_image(r), ("bwd", ("tall-dx", id(r)), r, r, 60, 1, 60, 300, 60))
    H, Cp, Dp = 3, 92, 4
    HC = H * Cp
    wn = torch.zeros(90, 270)
    Wcat, Ws_p = ops._plain_views(torch.zeros(Cp * (HC + 8) + HC * Cp + Dp * HC + Dp * 4 + Cp), H, Cp, Dp)[:2]
    assert (Wcat.stride(0), Ws_p.stride(0)) == (284, 92)
    node, upd = ops.wide_node_image(wn, W=Wcat), ops.wide_upd_image(wn, W=Ws_p)
    dagg, dx = ops.wide_dagg_image(wn, W=Ws_p), ops.wide_dx_image(wn, W=Wcat)
    assert ops.wide_dx_image.entry(wn) == dx[:3] and ops.lin_image.entry(w) == ops.lin_image(w, 16)[:3]      # what a hit looks up
    assert same(node, ("fwd", ("wide-img-node", id(wn)), wn, Wcat, Wcat.stride(0), 0, Cp, HC + 8, Cp))
    assert same(dagg, ("bwd", ("wide-img-dagg", id(wn)), wn, Ws_p, Ws_p.stride(0), 1, Cp, HC, Cp))
    assert same(upd, ("fwd", ("wide-img-upd", id(wn)), wn, Ws_p, Ws_p.stride(0), 0, HC, Cp, HC))
    assert same(dx, ("bwd", ("wide-img-dx", id(wn)), wn, Wcat, Wcat.stride(0), 1, HC + 8, Cp, HC + 8))
    # the prestage list of a tower is made of the same specs (CPU tensors stage nothing: see test_launch_saving_hints_are_host_logic)
    assert isinstance(node, tuple) and node.Kimg == Cp and node.table == "fwd"
