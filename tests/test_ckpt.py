"""Checkpoint layer: TensorBundle codec, Keras variable layout, save/load/resume."""
import os

import numpy as np
import pytest
import torch

from gnnqc import config as C
from gnnqc.ckpt import load_model, save_model
from gnnqc.ckpt.keras_layout import (build_from_keras, load_keras_optimizer, load_keras_weights,
                                     read_keras_metadata, write_keras_variables)
from gnnqc.ckpt.tensorbundle import bundle_entries, read_bundle, read_sstable, write_bundle, write_sstable
from gnnqc.models import create_model
from gnnqc.ops.optim import FlatAdam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ckpt")
REF_MODELS = ["model_cml", "model_cml_baseline", "model_soilnet", "model_soilnet_baseline"]
DATA = "variables.data-00000-of-00001"


@pytest.fixture(scope="session")
def REF(tmp_path_factory):
    """The reference's four trained checkpoints (``tests/golden/ref_ckpt``: keras_metadata.pb,
    fingerprint.pb, variables.index and the tensor data, stored in parts of 768 KiB) put together
    as SavedModel directories; the bundle reader's crc32c check covers the reassembled data."""
    import shutil
    root = tmp_path_factory.mktemp("ref_ckpt")
    for name in REF_MODELS:
        src, dst = os.path.join(GOLDEN, name), root / name
        os.makedirs(dst / "variables")
        for f in ("keras_metadata.pb", "fingerprint.pb", os.path.join("variables", "variables.index")):
            shutil.copyfile(os.path.join(src, f), dst / f)
        parts = sorted(f for f in os.listdir(os.path.join(src, "variables")) if f.startswith(DATA + ".part"))
        assert parts, src
        with open(dst / "variables" / DATA, "wb") as out:
            for f in parts:
                with open(os.path.join(src, "variables", f), "rb") as fh:
                    out.write(fh.read())
    return str(root)


def _model(ds="cml", baseline=False):
    pc = C.normalize_preproc(C.default(f"preprocessing_{ds}"))
    mc = C.default(f"model_{ds}")
    torch.manual_seed(0)
    return create_model(mc, pc, baseline=baseline), pc, mc


def test_sstable_roundtrip(tmp_path):
    items = [(f"key/{i:04d}".encode(), os.urandom(i % 37)) for i in range(700)] + [(b"", b"hdr")]
    p = str(tmp_path / "t.index")
    write_sstable(p, items, block_size=512)           # forces many data blocks + restarts
    got = read_sstable(p)
    assert got == sorted(items)


def test_bundle_roundtrip_dtypes(tmp_path):
    t = {"a/f32": np.random.randn(3, 5).astype(np.float32), "b/i64": np.arange(7, dtype=np.int64),
         "c/i32": np.array([1, 2, 3], np.int32), "d/str": "rolling_median", "e/scalar": np.float32(2.5),
         "f/bool": np.array([True, False])}
    prefix = str(tmp_path / "variables" / "variables")
    write_bundle(prefix, t)
    b = read_bundle(prefix)
    for k, v in t.items():
        if isinstance(v, str):
            assert b[k] == v.encode()
        else:
            np.testing.assert_array_equal(b[k], np.asarray(v))
    # corrupting one byte must trip the crc check
    data = prefix + ".data-00000-of-00001"
    raw = bytearray(open(data, "rb").read())
    raw[0] ^= 0xFF
    open(data, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="crc"):
        read_bundle(prefix)


@pytest.mark.parametrize("name", REF_MODELS)
def test_reference_checkpoint_layout(name, tmp_path, REF):
    """Every reference SavedModel loads into our module with matching shapes, and our
    writer reproduces its variables bit-exactly."""
    model, pc, mc = build_from_keras(os.path.join(REF, name))
    assert ("baseline" in name) == (type(model).__name__ == "BaselineClassifier")
    meta = read_keras_metadata(os.path.join(REF, name))
    assert meta["model_info"][:3] == [120, 60, 128] if "cml" in name else True
    write_keras_variables(model, str(tmp_path))
    ours = read_bundle(str(tmp_path / "variables" / "variables"))
    ref = read_bundle(os.path.join(REF, name, "variables", "variables"))
    for k, v in ours.items():
        if k.startswith("model_info") or k == "_CHECKPOINTABLE_OBJECT_GRAPH":   # (graph: own test)
            continue
        if isinstance(v, bytes):
            assert v == ref[k]
        else:
            np.testing.assert_array_equal(v, ref[k])
    # reference entries carry crc32c which read_bundle verified; Adam slots interleave m, v
    ents = bundle_entries(os.path.join(REF, name, "variables", "variables"))
    n_train = sum(1 for p in model.parameters() if p.requires_grad)
    assert sum(1 for k in ents if k.startswith("optimizer/_variables/")) == 2 * n_train


def test_reference_weights_forward_cpu(REF):
    """The trained reference CML GCN runs through our graph on CPU and gives finite,
    non-degenerate outputs (numerical parity with TF is unpinned: no TF / no data here)."""
    from gnnqc.data.synthetic import make_cml_raw
    from gnnqc.data.preprocessing import create_windows_dataset
    from gnnqc.data.store import DeviceStore
    model, pc, mc = build_from_keras(os.path.join(REF, "model_cml"))
    model.eval()
    ws = create_windows_dataset(pc, raw=make_cml_raw(n_sensors=10, n_minutes=3 * 1440, seed=3))
    store = DeviceStore(ws, model.model_normalization, pc.graph, device="cpu")
    batch = store.gather(torch.arange(min(16, ws.n_windows)))
    with torch.no_grad():
        p = model(batch.model_inputs("cml", False)).float()
    assert torch.isfinite(p).all() and p.std() > 0


def test_save_load_resume(tmp_path):
    model, pc, mc = _model()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    for p in model.parameters():
        if p.grad is not None:
            p.grad.normal_()
    opt.step()
    save_model(model, str(tmp_path), optimizer=opt, epoch=3, preproc_config=pc)
    assert os.path.exists(tmp_path / "variables" / "variables.index")
    m2, osd, meta = load_model(str(tmp_path), with_optimizer=True)
    assert meta["epoch"] == 3
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    # Keras-layout optimizer slots resume too
    m3, _, _ = _model()
    load_keras_weights(m3, str(tmp_path))
    opt3 = FlatAdam(m3.parameters(), lr=0.5)
    load_keras_optimizer(opt3, str(tmp_path))
    assert opt3.iterations == 1 and abs(opt3.lr - 1e-3) < 1e-9
    torch.testing.assert_close(opt3.m, opt.m)
    torch.testing.assert_close(opt3.v, opt.v)


@pytest.mark.parametrize("name", ["model_cml", "model_cml_baseline", "model_soilnet", "model_soilnet_baseline"])
def test_keras_metadata_matches_reference_structure(name, tmp_path, REF):
    """keras_metadata.pb written for a model built from the reference checkpoint has the
    reference's node paths, identifiers, class names and the key layer configs."""
    from gnnqc.ckpt.keras_meta import read_keras_metadata_pb, write_keras_metadata
    model, pc, mc = build_from_keras(os.path.join(REF, name))
    write_keras_metadata(model, str(tmp_path))
    ours = {n["node_path"]: n for n in read_keras_metadata_pb(str(tmp_path))}
    ref = {n["node_path"]: n for n in read_keras_metadata_pb(os.path.join(REF, name))}
    assert set(ours) == set(ref)

    def strip(v):   # shared_object_id numbering depends on Keras' global object counter
        if isinstance(v, dict):
            return {k: strip(x) for k, x in v.items() if k != "shared_object_id"}
        if isinstance(v, list):
            return [strip(x) for x in v]
        return v

    for path, r in ref.items():
        o = ours[path]
        assert o["identifier"] == r["identifier"], path
        rm, om = r["metadata"], o["metadata"]
        assert om["class_name"] == rm["class_name"], path
        for key in ("units", "return_sequences", "activation", "channels", "aggregate", "filter_1_size",
                    "n_stacks", "layer_type", "pool_size", "momentum", "epsilon", "num_thresholds"):
            if key in rm.get("config", {}):
                assert strip(om["config"].get(key)) == strip(rm["config"][key]), (path, key)
        if "build_input_shape" in rm and path != "root":
            assert om["build_input_shape"] == rm["build_input_shape"], path
    assert ours["root"]["metadata"]["training_config"]["loss"] == "binary_crossentropy"


def _graph_nodes(raw: bytes):
    from gnnqc.ckpt.tensorbundle import _proto_fields
    nodes = []
    for f, _, v in _proto_fields(raw):
        if f != 1:
            continue
        ch, at = [], []
        for f2, _, v2 in _proto_fields(v):
            if f2 == 1:
                d = {a: b for a, _, b in _proto_fields(v2)}
                ch.append((d.get(1, 0), d[2].decode()))
            elif f2 == 2:
                d = {a: b.decode() for a, _, b in _proto_fields(v2)}
                at.append(d)
        nodes.append((ch, at))
    return nodes


def _resolve(nodes, key):
    """Walk the object graph along the key's path; return the leaf's attribute keys."""
    node = 0
    for part in key.split("/.ATTRIBUTES/")[0].split("/"):
        node = dict((n, i) for i, n in nodes[node][0])[part]
    return [a[3] for a in nodes[node][1]]


def test_object_graph_and_fingerprint(tmp_path):
    """Saved checkpoints carry a TrackableObjectGraph resolving every key, and fingerprint.pb."""
    model, pc, mc = _model()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    save_model(model, str(tmp_path), optimizer=opt, epoch=0, preproc_config=pc)
    b = read_bundle(str(tmp_path / "variables" / "variables"))
    nodes = _graph_nodes(b["_CHECKPOINTABLE_OBJECT_GRAPH"])
    keys = [k for k in b if k.endswith("/.ATTRIBUTES/VARIABLE_VALUE")]
    assert len(keys) > 34
    for k in keys:
        assert _resolve(nodes, k) == [k]
    root_children = {n for _, n in nodes[0][0]}
    assert {"variables", "model_info", "optimizer"} <= root_children
    fp = (tmp_path / "fingerprint.pb").read_bytes()
    assert len(fp) > 40 and fp[0] == 0x08


def test_object_graph_paths_match_reference(REF):
    """Every variable key of the reference's own object graph resolves along the same path in
    the graph we write for the same architecture (the variable-bearing part of the graph)."""
    import tempfile
    ref = read_bundle(os.path.join(REF, "model_cml", "variables", "variables"))
    ref_nodes = _graph_nodes(ref["_CHECKPOINTABLE_OBJECT_GRAPH"])
    model, pc, mc = _model()
    with tempfile.TemporaryDirectory() as d:
        save_model(model, d, preproc_config=pc)
        ours = read_bundle(os.path.join(d, "variables", "variables"))
    nodes = _graph_nodes(ours["_CHECKPOINTABLE_OBJECT_GRAPH"])
    ref_keys = [k for k in ref if k.startswith(("variables/", "model_")) and k.endswith("VARIABLE_VALUE")]
    assert len(ref_keys) >= 34
    for k in ref_keys:
        assert _resolve(ref_nodes, k) == [k]
        assert _resolve(nodes, k) == [k]


def test_saved_model_pb_mirrors_object_graph(tmp_path):
    """saved_model.pb (best effort; no reference file exists to pin parity): one meta graph
    tagged 'serve', V2 saver, and a SavedObjectGraph whose nodes are the bundle's object graph node for
    node - same ids, same children - with variable records matching the stored tensors."""
    from gnnqc.ckpt.saved_model import read_saved_model_summary
    model, pc, mc = _model()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    save_model(model, str(tmp_path), optimizer=opt, epoch=0, preproc_config=pc)
    sm = read_saved_model_summary(str(tmp_path))
    assert sm["schema_version"] == 1 and len(sm["meta_graphs"]) == 1
    mg = sm["meta_graphs"][0]
    assert mg["tags"] == ["serve"] and mg["saver_version"] == 2 and mg["tensorflow_version"].startswith("2.11")
    b = read_bundle(str(tmp_path / "variables" / "variables"))
    og = _graph_nodes(b["_CHECKPOINTABLE_OBJECT_GRAPH"])
    ent = bundle_entries(str(tmp_path / "variables" / "variables"))
    assert ent["optimizer/_iterations/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == []     # scalars: shape [] like
    assert ent["optimizer/_learning_rate/.ATTRIBUTES/VARIABLE_VALUE"]["shape"] == []  # the reference's bundle
    nodes = mg["nodes"]
    assert len(nodes) == len(og)
    n_train = 0
    for i, (n, (ch, at)) in enumerate(zip(nodes, og)):
        assert n["children"] == ch, i
        if at:                                   # a variable node of the object graph
            key = at[0][3]
            assert n["kind"] == "variable" and n["name"] + "/.ATTRIBUTES/VARIABLE_VALUE" == key
            assert n["dtype"] == ent[key]["dtype"] and n.get("shape", []) == list(ent[key]["shape"]), key
            n_train += n["trainable"]
        else:
            assert n["kind"] == "user_object"
    assert nodes[0]["identifier"] == "_tf_keras_model"
    assert n_train == sum(1 for p in model.parameters() if p.requires_grad)
    # every checkpoint key resolves along the SavedObjectGraph's own children too
    for k in (k for k in b if k.endswith("/.ATTRIBUTES/VARIABLE_VALUE")):
        node = 0
        for part in k.split("/.ATTRIBUTES/")[0].split("/"):
            node = dict((nm, j) for j, nm in nodes[node]["children"])[part]
        assert nodes[node]["kind"] == "variable"
