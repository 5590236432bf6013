"""resnet_with_augmentation widths ([128, 64, 32, 32], linear size 128, 128 x 44 windows) without a GPU: the CPU oracle against the
reference fixtures of tools/make_aug_goldens.py, the drop-in model's state_dict layout, and the window length / frame shift that follow
config.FEAT['num_samples'] at call time."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from oracle import recipe, resnet_oracle as ro

AUG = dict(linear_layer_size=128, filter_sizes=[128, 64, 32, 32])


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "resnet_aug.npz"))


@pytest.fixture(scope="module")
def sd(g):
    return ro.to_torch_state(recipe.make_state(int(g["state_seed"]), filter_sizes=tuple(AUG["filter_sizes"]),
                                               linear_layer_size=AUG["linear_layer_size"]))


def test_oracle_state_and_drop_in_model_have_the_reference_layout(golden_dir):
    import models
    lay = json.load(open(os.path.join(golden_dir, "state_dict_layout_aug.json")))
    ref = [(k, tuple(s)) for k, s, dt in lay["entries"]]
    assert recipe.resnet_state_shapes(tuple(AUG["filter_sizes"]), AUG["linear_layer_size"]) == [(k, s) for (k, s), (_, _, dt) in
                                                                                                  zip(ref, lay["entries"]) if dt == "float32"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.ResNetBigger(dropout_rate=0.0, **AUG)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref
    assert [n for n, _ in m.named_parameters()] == lay["param_order"]
    assert sum(p.numel() for p in m.parameters()) == lay["n_params"]
    assert ("block1.0.shortcut.0.weight", (128, 64, 1, 1)) in ref   # the stride-1 projection shortcut


def test_oracle_eval_matches_the_reference(g, sd):
    x = torch.from_numpy(recipe.make_features(int(g["eval_seed"]), int(g["eval_batch"]), n_frames=int(g["n_frames"])))
    with torch.no_grad():
        probs = ro.forward(sd, x, train=False)
    np.testing.assert_allclose(probs.numpy(), g["eval_probs"], rtol=0, atol=2e-6)


def test_oracle_train_step_matches_the_reference(g, sd):
    B = int(g["train_batch"])
    x = torch.from_numpy(recipe.make_features(int(g["train_seed"]), B, n_frames=int(g["n_frames"])))
    t = torch.from_numpy(recipe.make_labels(int(g["label_seed"]), B))
    r = ro.train_step(sd, x, t)
    np.testing.assert_allclose(r["probs"].numpy(), g["train_probs"], atol=2e-6)
    assert abs(r["loss"] - float(g["loss"])) < 2e-6
    assert abs(r["grad_norm"] - float(g["total_norm"])) < 1e-4 * float(g["total_norm"])
    keys = [str(k) for k in g["grad_keys"]]
    assert keys == ro.param_keys(sd)
    for k, l2 in zip(keys, g["grad_l2"]):
        ours = float(r["grads"][k].double().norm())
        if k.endswith("conv1.bias") or k.endswith("conv2.bias"):
            assert ours < 1e-5 and l2 < 1e-5
        else:
            assert abs(ours - l2) <= 2e-3 * l2 + 1e-7, k
    for name in g.files:
        if name.startswith("grad::"):
            ref = g[name]
            got = r["grads"][name[6:]].numpy()
            assert np.linalg.norm(got - ref) <= 2e-3 * np.linalg.norm(ref), name
        if name.startswith("stat::"):
            np.testing.assert_allclose(r["new_sd"][name[6:]].numpy(), g[name], rtol=1e-5, atol=1e-6, err_msg=name)
        if name.startswith("delta::"):
            k = name[7:]
            ours = (r["new_sd"][k] - sd[k]).numpy()
            gref = g["grad::" + k]
            big = np.abs(gref) > 1e-2 * np.abs(gref).max()
            np.testing.assert_allclose(ours[big], g[name][big], rtol=0, atol=2e-6, err_msg=k)
    for k, d in zip(keys, g["delta_l2"]):
        if k.endswith("conv1.bias") or k.endswith("conv2.bias") or k in ("linear1.bias", "bn2.bias"):
            continue   # rounding-noise gradients: Adam moves them by +-lr at random on any two implementations
        assert abs(float((r["new_sd"][k] - sd[k]).double().norm()) - d) <= 2e-2 * d + 1e-6, k


@pytest.fixture
def feat128():
    import config
    old = dict(config.FEAT)
    config.FEAT["num_samples"] = 128
    yield
    config.FEAT.clear()
    config.FEAT.update(old)


def test_segment_tables_follow_num_samples(feat128):
    import segments
    assert segments.configured_frame_shift() == 1.0 / 128
    rows = [dict(audio_path="a.sph", sub_start="1.5", sub_duration="1.0", label="1"),
            dict(audio_path="a.sph", sub_start="0.01", sub_duration="0.5", label="0")]
    t = segments.table_from_rows(rows)
    assert t.frames_per_segment == 128
    assert list(t.first_frame) == [192, 1] and list(t.n_frames) == [128, 64]   # round(0.01 * 128) = 1, 0.5 s = 64 frames
    w = segments.whole_track_table(3 * 128 + 5, "a.sph")
    assert len(w) == 3 and list(w.first_frame) == [0, 128, 256]
    assert segments.SegmentTable(*(np.zeros(0, np.int32),) * 4, []).frames_per_segment == 128


def test_default_feat_keeps_100_frames():
    import segments
    assert segments.configured_frame_shift() == segments.FRAME_SHIFT == 0.01
    assert segments.table_from_rows([dict(audio_path="a", sub_start="0.5", sub_duration="2.0", label="1")]).frames_per_segment == 100


def test_inference_windows_follow_num_samples(feat128):
    import datasets
    feats = np.arange(300 * 44, dtype=np.float32).reshape(300, 44)
    ds = datasets.InferenceDataset(feats)
    assert ds.n_frames == 128
    assert ds[0].shape == (128, 44) and ds[250].shape == (128, 44) and not ds[250][50:].any()
