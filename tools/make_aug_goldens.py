#!/usr/bin/env python3
"""Reference fixtures for ResNetBigger at the resnet_with_augmentation widths ([128, 64, 32, 32], linear size 128) on
128 x 44 windows (FEAT['num_samples'] = 128): tests/golden/resnet_aug.npz and tests/golden/state_dict_layout_aug.json.

    python tools/make_aug_goldens.py [--ref <reference checkout>]

Runs where the reference is importable (it does not travel to the GPU box); it imports the reference's models.py the way
oracle/make_goldens.py does.  Weights: recipe.make_state(seed, filter_sizes=(128, 64, 32, 32), linear_layer_size=128); inputs:
recipe.make_features(seed, B, n_frames=128).  Deterministic: a second run writes the same bytes (single-threaded torch-CPU).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import recipe  # noqa: E402
from oracle.make_goldens import load_reference  # noqa: E402

AUG = dict(linear_layer_size=128, filter_sizes=[128, 64, 32, 32])
N_FRAMES = 128
STATE_SEED, EVAL_SEED, TRAIN_SEED, LABEL_SEED = 111, 212, 313, 414
EVAL_B, TRAIN_B = 4, 8
# full gradients / Adam deltas kept for these tensors (the stride-1 projection shortcut, a 128 -> 128 convolution, the stride-2 entries
# of the new shapes, the head); every tensor gets its L2 norm
FULL_KEYS = ["block1.0.shortcut.0.weight", "block1.0.shortcut.1.weight", "block1.1.conv1.weight", "block1.0.bn1.weight",
             "block2.0.shortcut.0.weight", "block4.0.conv1.weight", "block4.0.shortcut.0.weight", "bn2.weight", "linear1.weight",
             "linear2.weight"]


def build_model(models, seed):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.ResNetBigger(dropout_rate=0.0, **AUG)
    sd = recipe.make_state(seed, filter_sizes=tuple(AUG["filter_sizes"]), linear_layer_size=AUG["linear_layer_size"])
    full = m.state_dict()
    for k, v in sd.items():
        assert tuple(full[k].shape) == v.shape, k
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    models, _, _ = load_reference(args.ref)

    m = build_model(models, STATE_SEED)
    layout = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    with open(os.path.join(args.out, "state_dict_layout_aug.json"), "w") as f:
        json.dump({"n_params": sum(p.numel() for p in m.parameters()), "entries": layout,
                   "param_order": [k for k, _ in m.named_parameters()]}, f, indent=0)

    save = dict(state_seed=STATE_SEED, eval_seed=EVAL_SEED, train_seed=TRAIN_SEED, label_seed=LABEL_SEED, eval_batch=EVAL_B,
                train_batch=TRAIN_B, n_frames=N_FRAMES)
    # eval-mode probabilities (running statistics of the initial state)
    m.eval()
    with torch.no_grad():
        save["eval_probs"] = m(torch.from_numpy(recipe.make_features(EVAL_SEED, EVAL_B, n_frames=N_FRAMES))).numpy()

    # one train step: forward (batch statistics), BCE, backward, clip_grad_norm_(1.0), Adam (train.py:261-297)
    m = build_model(models, STATE_SEED)
    m.train()
    x = torch.from_numpy(recipe.make_features(TRAIN_SEED, TRAIN_B, n_frames=N_FRAMES))
    t = torch.from_numpy(recipe.make_labels(LABEL_SEED, TRAIN_B)).float()
    opt = torch.optim.Adam(m.parameters())
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    out = m(x).squeeze()
    loss = torch.nn.BCELoss()(out, t)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    total_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    after = {k: v.detach().clone() for k, v in m.named_parameters()}
    save.update(train_probs=out.detach().numpy(), loss=np.float64(loss.item()), total_norm=np.float64(float(total_norm)),
                grad_keys=np.array(list(grads)), grad_l2=np.array([float(g.double().norm()) for g in grads.values()]),
                delta_l2=np.array([float((after[k] - before[k]).double().norm()) for k in grads]))
    for k in FULL_KEYS:
        save["grad::" + k] = grads[k].numpy()
        if grads[k].numel() <= 20000:   # (the 128 -> 128 convolution's 147 k deltas: L2 norm only)
            save["delta::" + k] = (after[k] - before[k]).numpy()
    for k, v in m.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            save["stat::" + k] = v.numpy()
    np.savez_compressed(os.path.join(args.out, "resnet_aug.npz"), **save)
    for fn in ("resnet_aug.npz", "state_dict_layout_aug.json"):
        print(f"  {fn:32s} {os.path.getsize(os.path.join(args.out, fn)):>9d} B")


if __name__ == "__main__":
    main()
