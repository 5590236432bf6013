"""ResNetBigger at the resnet_with_augmentation widths ([128, 64, 32, 32], linear size 128) on 128 x 44 windows, on the MI355X.

Per operator (every convolution shape these widths add, forward / data gradient / weight gradient, train and eval epilogues, and
the BatchNorm backward at 128 channels) against torch-CPU float64 at the per-operator bars of tests/test_resnet_gpu.py; the model
end to end against tests/golden/resnet_aug.npz (tools/make_aug_goldens.py, the reference's models.py) and the CPU oracle; the
sliding-window path; the plumbing that makes the window length follow config.FEAT['num_samples'].
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe, resnet_oracle as ro

pytestmark = pytest.mark.gpu

AUG = dict(linear_layer_size=128, filter_sizes=[128, 64, 32, 32])
T_FRAMES = 128
P_TOL = 2e-5
G_L2, G_MAX = 2e-2, 5e-2
OP_TOL = 2e-4      # per-operator bar of the convolutions (relative L2 and max |diff| over max |ref|), float64 reference
BN_TOL = 1e-5      # ... of the BatchNorm backward (max |diff| over max |ref|)


def noise_grad(name):
    return name.endswith("conv1.bias") or name.endswith("conv2.bias") or name in ("linear1.bias", "bn2.bias")


def assert_grad_close(got, ref, name, l2_tol=G_L2, max_tol=G_MAX):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    mx = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert l2 <= l2_tol and mx <= max_tol, (name, l2, mx)


def op_close(got, ref, what):
    assert_grad_close(got.double().cpu().numpy(), ref.double().numpy(), what, OP_TOL, OP_TOL)


def _h():
    import _hip
    return _hip


def act_rows(B, H, W):
    return B * (H + 1) * (W + 1) + (W + 1) + 1


def to_pnhwc(x):
    B, C, H, W = x.shape
    buf = torch.zeros(act_rows(B, H, W) * C)
    buf[:B * (H + 1) * (W + 1) * C].view(B, H + 1, W + 1, C)[:, 1:, 1:, :] = x.float().permute(0, 2, 3, 1)
    return buf.cuda()


def from_pnhwc(buf, B, C, H, W):
    return buf[:B * (H + 1) * (W + 1) * C].view(B, H + 1, W + 1, C)[:, 1:, 1:, :].permute(0, 3, 1, 2).cpu()


def borders_are_zero(buf, B, C, H, W):
    n = B * (H + 1) * (W + 1) * C
    body = buf[:n].view(B, H + 1, W + 1, C)
    return float(body[:, 0].abs().max()) == 0 and float(body[:, :, 0].abs().max()) == 0 and float(buf[n:].abs().max()) == 0


def build_model(seed=111, dropout=0.0):
    import models
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.ResNetBigger(dropout_rate=dropout, **AUG)
    sd = recipe.make_state(seed, filter_sizes=tuple(AUG["filter_sizes"]), linear_layer_size=AUG["linear_layer_size"])
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    m.set_device("cuda")
    return m, ro.to_torch_state(sd)


def _pack(lib, h, w, cout, cin, taps, st):
    wg = w.float().cuda()
    wt_f = torch.zeros(int(lib.lad_conv_packed_weight_floats(cout, cin, taps, 0)), device="cuda")
    wt_d = torch.zeros(int(lib.lad_conv_packed_weight_floats(cout, cin, taps, 1)), device="cuda")
    h.check(lib.lad_conv_pack_weights(h.ptr(wg), cout, cin, taps, 0, h.ptr(wt_f), st))
    h.check(lib.lad_conv_pack_weights(h.ptr(wg), cout, cin, taps, 1, h.ptr(wt_d), st))
    return wt_f, wt_d


# ------------------------------------------------------------------------------------------ per operator
# (B, H, W): the level-1 geometry of one window (B = 1) and of three (3 * 129 * 45 rows: the last 128-row tile ends mid-tile), and a
# small odd image
S1_GEOMS = [(1, 128, 44), (3, 128, 44), (5, 13, 7)]


@pytest.mark.parametrize("cin,cout,taps", [(64, 128, 9), (128, 128, 9), (64, 128, 1)])
@pytest.mark.parametrize("B,H,W", S1_GEOMS)
def test_stride1_convolutions_of_block1(cin, cout, taps, B, H, W):
    """lad_conv_fwd (+ bias, + residual addend, BatchNorm partials), its data gradient (the swapped instance), lad_conv_wgrad (the
    sliced weight gradient) and lad_conv_fwd_eval, against float64."""
    h = _h()
    lib = h.lib()
    st = h.stream_handle()
    g = torch.Generator().manual_seed(cin + cout + taps + B)
    k = 3 if taps == 9 else 1
    pad = k // 2
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * 0.05
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    add = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
    x, w, bias, add = (t.float().double() for t in (x, w, bias, add))   # exactly representable in fp32
    wt_f, wt_d = _pack(lib, h, w, cout, cin, taps, st)
    xin = to_pnhwc(x)
    out = torch.full((act_rows(B, H, W) * cout,), 9.0, device="cuda")
    n_tiles = int(lib.lad_conv_num_tiles(B, H, W))
    part = torch.zeros(n_tiles * 2 * cout, device="cuda")
    bg, addg = bias.float().cuda(), to_pnhwc(add)
    h.check(lib.lad_conv_fwd(h.ptr(xin), h.ptr(wt_f), h.ptr(bg), h.ptr(addg), h.ptr(out), h.ptr(part), B, H, W, cin, cout, taps, st))
    ref = F.conv2d(x, w, bias, padding=pad) + add
    op_close(from_pnhwc(out, B, cout, H, W), ref, "fwd")
    assert borders_are_zero(out, B, cout, H, W)
    ps = part.view(n_tiles, 2, cout).double().sum(0).cpu()
    assert torch.allclose(ps[0], ref.sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(ps[1], (ref ** 2).sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
    # data gradient
    dout = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64).float().double()
    doutg = to_pnhwc(dout)
    dx = torch.full((act_rows(B, H, W) * cin,), 7.0, device="cuda")
    h.check(lib.lad_conv_fwd(h.ptr(doutg), h.ptr(wt_d), None, None, h.ptr(dx), None, B, H, W, cout, cin, taps, st))
    op_close(from_pnhwc(dx, B, cin, H, W), F.conv_transpose2d(dout, w, padding=pad), "dgrad")
    assert borders_are_zero(dx, B, cin, H, W)
    # weight + bias gradient
    ws = torch.zeros(int(lib.lad_conv_wgrad_workspace_floats(cin, cout, taps)), device="cuda")
    dw = torch.zeros(cout, cin, k, k, device="cuda")
    db = torch.zeros(cout, device="cuda")
    h.check(lib.lad_conv_wgrad(h.ptr(xin), h.ptr(doutg), h.ptr(ws), h.ptr(dw), h.ptr(db), B, H, W, cin, cout, taps, st))
    wr = w.clone().requires_grad_(True)
    (F.conv2d(x, wr, None, padding=pad) * dout).sum().backward()
    op_close(dw, wr.grad, "wgrad")
    op_close(db, dout.sum((0, 2, 3)), "bias grad")
    # eval epilogue: relu(conv * scale + shift + addend)
    scale = (torch.rand(cout, generator=g, dtype=torch.float64) + 0.5).float().double()
    shift = torch.randn(cout, generator=g, dtype=torch.float64).float().double()
    ev = torch.full((act_rows(B, H, W) * cout,), 9.0, device="cuda")
    sg, shg = scale.float().cuda(), shift.float().cuda()
    h.check(lib.lad_conv_fwd_eval(h.ptr(xin), h.ptr(wt_f), h.ptr(sg), h.ptr(shg), h.ptr(addg), h.ptr(ev), B, H, W, cin, cout, taps, 1, st))
    conv = F.conv2d(x, w, None, padding=pad)
    op_close(from_pnhwc(ev, B, cout, H, W), F.relu(conv * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + add), "eval")
    assert borders_are_zero(ev, B, cout, H, W)


@pytest.mark.parametrize("cin,cout", [(128, 64), (32, 32)])
@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("B,H,W", [(1, 128, 44), (3, 32, 11), (2, 25, 13)])
def test_stride2_convolutions_of_block2_and_block4(cin, cout, taps, B, H, W):
    """lad_conv_s2_fwd (+ partials), lad_conv_s2_fwd_eval, lad_conv_s2_dgrad (the 1x1 accumulates) and lad_conv_s2_wgrad (sliced
    at 128 input channels) against float64."""
    h = _h()
    lib = h.lib()
    st = h.stream_handle()
    g = torch.Generator().manual_seed(cin * 3 + cout + taps + H)
    k = 3 if taps == 9 else 1
    pad = k // 2
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).float().double()
    w = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * 0.05).float().double()
    bias = torch.randn(cout, generator=g, dtype=torch.float64).float().double()
    wt_f, wt_d = _pack(lib, h, w, cout, cin, taps, st)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xin = to_pnhwc(x)
    out = torch.full((act_rows(B, Ho, Wo) * cout,), 5.0, device="cuda")
    n_tiles = int(lib.lad_conv_num_tiles(B, Ho, Wo))
    part = torch.zeros(n_tiles * 2 * cout, device="cuda")
    bg = bias.float().cuda()
    h.check(lib.lad_conv_s2_fwd(h.ptr(xin), h.ptr(wt_f), h.ptr(bg), h.ptr(out), h.ptr(part), B, H, W, cin, cout, taps, st))
    ref = F.conv2d(x, w, bias, stride=2, padding=pad)
    op_close(from_pnhwc(out, B, cout, Ho, Wo), ref, "s2 fwd")
    assert borders_are_zero(out, B, cout, Ho, Wo)
    ps = part.view(n_tiles, 2, cout).double().sum(0).cpu()
    assert torch.allclose(ps[0], ref.sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
    scale = (torch.rand(cout, generator=g, dtype=torch.float64) + 0.5).float().double()
    shift = torch.randn(cout, generator=g, dtype=torch.float64).float().double()
    ev = torch.full((act_rows(B, Ho, Wo) * cout,), 5.0, device="cuda")
    sg, shg = scale.float().cuda(), shift.float().cuda()   # (held: the launch is asynchronous)
    h.check(lib.lad_conv_s2_fwd_eval(h.ptr(xin), h.ptr(wt_f), h.ptr(sg), h.ptr(shg), h.ptr(ev), B, H, W, cin, cout, taps, 1, st))
    conv = F.conv2d(x, w, None, stride=2, padding=pad)
    op_close(from_pnhwc(ev, B, cout, Ho, Wo), F.relu(conv * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), "s2 eval")
    # gradients
    dout = torch.randn(B, cout, Ho, Wo, generator=g, dtype=torch.float64).float().double()
    doutg = to_pnhwc(dout)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (F.conv2d(xr, wr, None, stride=2, padding=pad) * dout).sum().backward()
    base = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).float().double()
    dx = to_pnhwc(base) if taps == 1 else torch.full((act_rows(B, H, W) * cin,), 0.0, device="cuda")
    h.check(lib.lad_conv_s2_dgrad(h.ptr(doutg), h.ptr(wt_d), h.ptr(dx), B, H, W, cin, cout, taps, 1 if taps == 1 else 0, st))
    op_close(from_pnhwc(dx, B, cin, H, W), xr.grad + (base if taps == 1 else 0), "s2 dgrad")
    assert borders_are_zero(dx, B, cin, H, W)
    ws = torch.zeros(int(lib.lad_conv_s2_wgrad_workspace_floats(cin, cout, taps)), device="cuda")
    dw = torch.zeros(cout, cin, k, k, device="cuda")
    db = torch.zeros(cout, device="cuda")
    h.check(lib.lad_conv_s2_wgrad(h.ptr(xin), h.ptr(doutg), h.ptr(ws), h.ptr(dw), h.ptr(db), B, H, W, cin, cout, taps, st))
    op_close(dw, wr.grad, "s2 wgrad")
    op_close(db, dout.sum((0, 2, 3)), "s2 bias grad")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batchnorm_backward_at_128_channels(mode):
    """lad_bn_finalize -> lad_bn_act -> lad_bn_bwd at 128 channels (mode 0: dx; 1: + identity shortcut; 2: + projection shortcut
    BatchNorm) against float64 autograd, with the GPU's own ReLU decisions."""
    h = _h()
    lib = h.lib()
    st = h.stream_handle()
    C, B, H, W = 128, 3, 16, 11
    g = torch.Generator().manual_seed(128 + mode)
    rows, cnt = act_rows(B, H, W), B * H * W
    x = torch.randn(B, C, H, W, generator=g) * 2 + 3
    xs = torch.randn(B, C, H, W, generator=g) - 1
    res = torch.randn(B, C, H, W, generator=g)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    sgam, sbet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, C, H, W, generator=g)
    keep = []

    def dev(t):
        keep.append(t.cuda())
        return keep[-1]

    def coef_of(t, ga, be):
        stats = torch.stack([t.double().sum((0, 2, 3)), (t.double() ** 2).sum((0, 2, 3))]).float().reshape(-1)
        rm, rv, coef = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros(6 * C, device="cuda")
        h.check(lib.lad_bn_finalize(h.ptr(dev(stats)), 1, C, cnt, h.ptr(dev(ga)), h.ptr(dev(be)), h.ptr(rm), h.ptr(rv), 0.1, h.ptr(coef), st))
        return coef

    coef, scoef = coef_of(x, gam, bet), coef_of(xs, sgam, sbet)
    xg, xsg, rg = to_pnhwc(x), to_pnhwc(xs), to_pnhwc(res)
    y = torch.zeros(rows * C, device="cuda")
    resp, rcp = {0: (None, None), 1: (h.ptr(rg), None), 2: (h.ptr(xsg), h.ptr(scoef))}[mode]
    h.check(lib.lad_bn_act(h.ptr(xg), h.ptr(coef), resp, rcp, h.ptr(y), B, H, W, C, 1, st))
    x64, xs64 = x.double().requires_grad_(True), xs.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    sg64, sb64 = sgam.double().requires_grad_(True), sbet.double().requires_grad_(True)
    z = F.batch_norm(x64, None, None, g64, b64, training=True, eps=1e-5)
    if mode == 2:
        z = z + F.batch_norm(xs64, None, None, sg64, sb64, training=True, eps=1e-5)
    elif mode == 1:
        z = z + res.double()
    got = from_pnhwc(y, B, C, H, W).double()
    assert (got - F.relu(z).detach()).abs().max() < 2e-6 * z.abs().max()
    (z * (got > 0) * dy.double()).sum().backward()
    dx, aux = torch.zeros(rows * C, device="cuda"), torch.zeros(rows * C, device="cuda")
    dg, db, dsg, dsb = (torch.zeros(C, device="cuda") for _ in range(4))
    ws = torch.zeros(int(lib.lad_bn_bwd_workspace_floats(C)), device="cuda")
    bcoef = torch.zeros(8 * C, device="cuda")
    sh = mode == 2
    h.check(lib.lad_bn_bwd(h.ptr(dev(to_pnhwc(dy))), h.ptr(y), h.ptr(xg), h.ptr(coef), h.ptr(dev(gam)), h.ptr(xsg) if sh else None,
                           h.ptr(scoef) if sh else None, h.ptr(dev(sgam)) if sh else None, h.ptr(dx), h.ptr(aux) if mode else None,
                           h.ptr(dg), h.ptr(db), h.ptr(dsg) if sh else None, h.ptr(dsb) if sh else None, h.ptr(ws), h.ptr(bcoef), None, 0,
                           B, H, W, C, 1, mode, st))

    def close(a, b):
        b = b.double()
        assert (a.double().cpu() - b).abs().max() <= BN_TOL * b.abs().max(), float((a.double().cpu() - b).abs().max() / b.abs().max())

    close(from_pnhwc(dx, B, C, H, W), x64.grad)
    close(dg, g64.grad)
    close(db, b64.grad)
    if mode == 2:
        close(from_pnhwc(aux, B, C, H, W), xs64.grad)
        close(dsg, sg64.grad)
        close(dsb, sb64.grad)
    if mode == 1:
        close(from_pnhwc(aux, B, C, H, W), dy.double() * (got > 0))


# ------------------------------------------------------------------------------------------ the model end to end
def test_kernel_selection_is_exact_f32_only():
    m, _ = build_model()
    eng = m.engine
    assert not eng.base_widths
    assert not any(getattr(eng, k) for k in eng.KERNEL_OPTIONS)
    m.train()
    x = torch.from_numpy(recipe.make_features(1, 2, n_frames=T_FRAMES)).cuda()
    eng.forward(x, train=True, labels=torch.zeros(2, dtype=torch.int32, device="cuda"))
    for b in eng._last_train_plan["blocks"]:
        for cs in (b.conv1, b.conv2, b.sc_conv):
            if cs is not None:
                assert not cs.b3 and not cs.s2b3, cs.name
    for b in eng._last_train_plan["schedule"].blocks:
        assert all(c.arith == "f32" and c.wgrad == "f32" for c in (b.conv1, b.conv2, b.sc) if c is not None)


def test_eval_probabilities_match_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "resnet_aug.npz"))
    m, sd = build_model(int(g["state_seed"]))
    m.eval()
    x = torch.from_numpy(recipe.make_features(int(g["eval_seed"]), int(g["eval_batch"]), n_frames=T_FRAMES)).cuda()
    with torch.no_grad():
        probs = m(x)
    np.testing.assert_allclose(probs.cpu().numpy(), g["eval_probs"], rtol=0, atol=P_TOL)
    one = m.predict(x[:1]).cpu().numpy()                                  # B = 1
    np.testing.assert_allclose(one, g["eval_probs"][:1, 0], rtol=0, atol=P_TOL)


def test_train_step_matches_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "resnet_aug.npz"))
    B = int(g["train_batch"])
    m, sd = build_model(int(g["state_seed"]))
    m.train()
    x = torch.from_numpy(recipe.make_features(int(g["train_seed"]), B, n_frames=T_FRAMES)).cuda()
    t = torch.from_numpy(recipe.make_labels(int(g["label_seed"]), B)).cuda()
    eng = m.engine
    probs = eng.forward(x, train=True, labels=t).clone()
    np.testing.assert_allclose(probs.cpu().numpy(), g["train_probs"], rtol=0, atol=P_TOL)
    from engine import metrics_from_counters
    assert abs(metrics_from_counters(eng.metrics().cpu().numpy())[0] - float(g["loss"])) < P_TOL
    eng.backward(None)
    grads = {k: v.cpu().numpy().copy() for k, v in eng.grad_views().items()}
    keys = [str(k) for k in g["grad_keys"]]
    assert keys == [n for n, _ in m.named_parameters()]
    total = np.sqrt(sum(float((grads[k].astype(np.float64) ** 2).sum()) for k in keys))
    assert abs(total - float(g["total_norm"])) < 1e-3 * float(g["total_norm"])
    for k, l2 in zip(keys, g["grad_l2"]):
        ours = float(np.linalg.norm(grads[k].astype(np.float64)))
        if noise_grad(k):
            assert ours < 1e-4, (k, ours)
        else:
            assert abs(ours - l2) <= 2e-2 * l2 + 1e-7, (k, ours, l2)
    for k in g.files:
        if k.startswith("grad::") and not noise_grad(k[6:]):
            assert_grad_close(grads[k[6:]], g[k], k[6:])
        if k.startswith("stat::"):
            got = dict(m.named_buffers())[k[6:]].cpu().numpy()
            np.testing.assert_allclose(got, g[k], rtol=1e-4, atol=1e-6, err_msg=k)
    before = {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    eng.reset_optimizer()
    norm = eng.clip_and_step()
    assert abs(float(norm.cpu()) - float(g["total_norm"])) < 1e-3 * float(g["total_norm"])
    for k in g.files:
        if k.startswith("delta::") and not noise_grad(k[7:]):
            name = k[7:]
            ours = dict(m.named_parameters())[name].detach().cpu().numpy() - before[name]
            gref = g["grad::" + name]
            big = np.abs(gref) > 1e-2 * np.abs(gref).max()
            np.testing.assert_allclose(ours[big], g[k][big], rtol=0, atol=2e-5, err_msg=name)


def test_gradients_with_the_same_relu_decisions_at_batch_64():
    """With the engine's ReLU decisions imposed on the oracle both compute the same function: 1e-4 relative L2 per tensor."""
    B = 64
    m, sd = build_model(121)
    m.train()
    xf = recipe.make_features(122, B, n_frames=T_FRAMES)
    tl = recipe.make_labels(123, B)
    eng = m.engine
    probs = eng.forward(torch.from_numpy(xf).cuda(), train=True, labels=torch.from_numpy(tl).cuda()).clone()
    eng.backward(None)
    rm = ro.train_step(sd, torch.from_numpy(xf), torch.from_numpy(tl), relu_masks=eng.export_relu_masks())
    np.testing.assert_allclose(probs.cpu().numpy(), rm["probs"].numpy(), rtol=0, atol=P_TOL)
    for k, gv in eng.grad_views().items():
        if noise_grad(k):
            continue
        ref = rm["grads"][k].double().numpy()
        l2 = np.linalg.norm(gv.cpu().double().numpy() - ref) / np.linalg.norm(ref)
        assert l2 <= 1e-4, (k, l2)
    for k, v in m.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(v.cpu().numpy(), rm["new_sd"][k].numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_graphed_train_step_equals_eager():
    B = 16
    m1, _ = build_model(131)
    m2, _ = build_model(131)
    m1.train(); m2.train()
    m1.engine.reset_optimizer(); m2.engine.reset_optimizer()
    step = m2.make_graphed_train_step(B, n_frames=T_FRAMES, drop_masks=None)
    for k in range(2):
        x = torch.from_numpy(recipe.make_features(140 + k, B, n_frames=T_FRAMES)).cuda()
        t = torch.from_numpy(recipe.make_labels(150 + k, B)).cuda()
        me = m1.train_step(x, t, drop_masks=None).clone()
        mg = step(x, t).clone()
        assert torch.equal(me, mg), (k, me, mg)
    assert torch.equal(m1.engine.flat_param(), m2.engine.flat_param())
    for (n1, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(b1, b2), n1


# ------------------------------------------------------------------------------------------ inference
def _track(T, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, 44, generator=g) * 2.0 - 8.0).cuda()


def test_sliding_windows_fp32_equal_per_window_predict_and_the_oracle():
    """A 20 s track at 128 frames per second: predict_windows (stream on: these widths have no stride-1 block before the first
    projection, so every window runs the whole model) equals model.predict on the materialised windows, bit for bit, and the
    oracle on the first, the last and the windows either side of a PREDICT_CHUNK boundary."""
    import engine
    m, sd = build_model(161)
    m.eval()
    T = 20 * 128 + 17
    fg = _track(T)
    got = m.engine.predict_windows(fg, n_frames=T_FRAMES).clone()
    chunk = engine.PREDICT_CHUNK["fp32"]
    padded = torch.cat([fg, torch.zeros(T_FRAMES - 1, 44, device="cuda")])
    wins = padded.unfold(0, T_FRAMES, 1).permute(0, 2, 1)[:T]             # window i = frames [i, i + 128), zero-padded at the end
    per = torch.cat([m.predict(wins[s:s + 256].contiguous().unsqueeze(1)).clone() for s in range(0, T, 256)])
    assert torch.equal(got, per)
    pick = [0, chunk - 1, chunk, T - 1]
    with torch.no_grad():
        ref = ro.forward(sd, wins[pick].unsqueeze(1).cpu(), train=False).view(-1).numpy()
    np.testing.assert_allclose(got[pick].cpu().numpy(), ref, rtol=0, atol=P_TOL)
    part = m.engine.predict_windows(fg, n_frames=T_FRAMES, chunk=300, start=chunk - 7, stop=T)
    assert torch.equal(part, got[chunk - 7:])


def test_fp16_inference_at_these_widths_is_refused():
    m, _ = build_model()
    m.eval()
    with pytest.raises(ValueError, match="64, 32, 16, 16"):
        m.engine.predict_windows(_track(400), n_frames=T_FRAMES, precision="fp16")


# ------------------------------------------------------------------------------------------ plumbing at FEAT['num_samples'] = 128
@pytest.fixture
def feat128():
    import config
    old = dict(config.FEAT)
    config.FEAT["num_samples"] = 128
    yield
    config.FEAT.clear()
    config.FEAT.update(old)


def test_extractor_and_windows_follow_num_samples(feat128):
    import config
    import datasets
    from utils import get_feat_extractor
    ex = get_feat_extractor(config.FEAT["num_samples"], config.FEAT["num_filters"])
    pcm = torch.from_numpy(recipe.make_clips(7, 3).reshape(-1)).cuda()
    feats = ex.extract_long(pcm)
    assert abs(feats.shape[0] - 3 * 128) <= 1, feats.shape              # hop 125 samples: 128 frames per second
    ds = datasets.InferenceDataset(feats)
    assert ds.n_frames == 128 and ds[0].shape == (128, 44)
    assert ds.batch(0, 5).shape == (5, 128, 44)


def test_segment_laughter_end_to_end_with_a_checkpoint_of_these_widths(feat128, tmp_path):
    import wave
    import config
    import segment_laughter
    import torch_utils
    m, _ = build_model(171)
    state = torch_utils.make_state_dict(m, None, 0, 0, float("inf"))       # what train.py writes (train.py:130-131)
    torch_utils.save_checkpoint(state, is_best=True, checkpoint=str(tmp_path / "ckpt"))
    sr, secs = 16000, 6
    pcm = (recipe.make_clips(9, secs).reshape(-1) * 32767).clip(-32768, 32767).astype(np.int16)
    wav = tmp_path / "track.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())
    model = segment_laughter.build_model("resnet_with_augmentation", str(tmp_path / "ckpt"), torch.device("cuda"))
    for (n, p), (_, q) in zip(model.state_dict().items(), m.state_dict().items()):
        assert torch.equal(p.cpu(), q.cpu()), n
    probs, length = segment_laughter.predict_file(model, str(wav))
    assert abs(length - secs) < 1e-6 and abs(len(probs) - secs * 128) <= 1
    assert np.all(np.isfinite(probs)) and probs.min() >= 0 and probs.max() <= 1
    segment_laughter.main(["--config", "resnet_with_augmentation", "--model_path", str(tmp_path / "ckpt"), "--input_audio_file", str(wav),
                           "--output_dir", str(tmp_path / "out"), "--thresholds", "0.0,0.5", "--min_lengths", "0.0"])
    assert (tmp_path / "out" / "t_0.0" / "l_0.0" / "track.TextGrid").exists()
    assert config.FEAT["num_samples"] == 128
