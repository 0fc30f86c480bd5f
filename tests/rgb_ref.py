"""fp64 reference of the RGB network's CNN front-end (torch-CPU float64 conv2d / relu / max_pool2d with autograd), composed with the
numpy LSTM / Dense / CTC oracle for whole train steps.  Layouts are Keras' channels-last ones."""
import numpy as np
import torch

from oracle import keras_ref as kr


def conv_pool(x, W, b):
    """x (N, H, W, Cin), W (k, k, Cin, Cout), b (Cout,) torch float64 -> pooled (N, Hp, Wp, Cout): valid conv, bias, ReLU, 2x2 floor
    max-pool (torch's max_pool2d also routes a tie to the first maximum in row-major window order)."""
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), b)
    y = torch.nn.functional.max_pool2d(torch.relu(y), 2, 2)
    return y.permute(0, 2, 3, 1)


def conv_layer(x, W, b, dY):
    """One layer alone: pooled output and the gradients (dX, dW, db) of sum(pooled * dY)."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    bt = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    y = conv_pool(xt, Wt, bt)
    (y * torch.tensor(np.asarray(dY, np.float64))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()


def conv_layer_routed(x, W, b, dY, code):
    """One layer's fp64 pre-activation windows and its gradients for a GIVEN pool routing `code` (uint8 (N, Hp, Wp, Cout): window
    position dy*2+dx, 255 = none) - the routing an f32 forward chose; near-ties (two window values within f32 rounding) may
    legitimately route differently in fp64.  Returns (pre (N, Hp, Wp, Cout, 4) fp64, dX, dW, db)."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    bt = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    y = torch.nn.functional.conv2d(xt.permute(0, 3, 1, 2), Wt.permute(3, 2, 0, 1), bt).permute(0, 2, 3, 1)   # (N, Ho, Wo, C)
    N, Hp, Wp, Cn = code.shape
    win = y[:, :2 * Hp, :2 * Wp, :].reshape(N, Hp, 2, Wp, 2, Cn).permute(0, 1, 3, 5, 2, 4).reshape(N, Hp, Wp, Cn, 4)
    sel = np.zeros((N, Hp, Wp, Cn, 4))
    cd = np.asarray(code).astype(np.int64)
    for d in range(4):
        sel[..., d] = (cd == d)
    (win * torch.tensor(sel * np.asarray(dY, np.float64)[..., None])).sum().backward()
    return win.detach().numpy(), xt.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()


def conv_windows(x, W, b):
    """One layer's fp64 pre-activation windows (N, Hp, Wp, Cout, 4) alone, without autograd: what conv_layer_routed returns first.
    Their ReLU maximum over the last axis is conv_pool's output."""
    with torch.no_grad():
        xt, Wt, bt = (torch.tensor(np.asarray(a, np.float64)) for a in (x, W, b))
        y = torch.nn.functional.conv2d(xt.permute(0, 3, 1, 2), Wt.permute(3, 2, 0, 1), bt).permute(0, 2, 3, 1)
        N, Ho, Wo, Cn = y.shape
        Hp, Wp = Ho // 2, Wo // 2
        win = y[:, :2 * Hp, :2 * Wp, :].reshape(N, Hp, 2, Wp, 2, Cn).permute(0, 1, 3, 5, 2, 4).reshape(N, Hp, Wp, Cn, 4)
    return win.numpy()


def reference_code(pre):
    """fp64 routing of pre-activation windows (N, Hp, Wp, C, 4) and each window's gap between its two largest ReLU values."""
    r = np.maximum(pre, 0.0)
    code = np.where(r.max(-1) > 0, r.argmax(-1), 255)
    srt = np.sort(r, axis=-1)
    return code, srt[..., -1] - srt[..., -2]


def frontend_names(spec):
    s = spec["streams"][0]
    return s["name"], [c["name"] for c in s["frontend"]["layers"]]


def routed_pool(x, W, b, code):
    """conv + bias + ReLU, pooled by a GIVEN routing code (N, Hp, Wp, Cout) (255 = a ReLU-zero window: 0)."""
    y = torch.relu(torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), b)).permute(0, 2, 3, 1)
    N, Hp, Wp, Cn = code.shape
    win = y[:, :2 * Hp, :2 * Wp, :].reshape(N, Hp, 2, Wp, 2, Cn).permute(0, 1, 3, 5, 2, 4).reshape(N, Hp, Wp, Cn, 4)
    cd = torch.tensor(np.asarray(code).astype(np.int64))
    out = torch.gather(win, 4, torch.clamp(cd, max=3).unsqueeze(-1)).squeeze(-1)
    return torch.where(cd == 255, torch.zeros_like(out), out)


def loss_and_grads(spec, w, x, labels, input_length, label_length, codes=None):
    """Mean CTC loss, per-sample losses, every gradient and the posteriors of one RGB train step (no dropout: every rate is 0).
    spec: NetworkSpec.to_dict() of one front-end stream with a stacked BiLSTM [+ residual add]; x (B, T, h, w, c).
    codes: {conv layer name: pool routing (N, Hp, Wp, Cout)} of an f32 forward - its window choices are used instead of the fp64
    ones (they differ only at near-ties, where both are right)."""
    name, convs = frontend_names(spec)
    s = spec["streams"][0]
    B, T = x.shape[:2]
    ws = {c: (torch.tensor(np.asarray(w["%s/%s/W" % (name, c)], np.float64), requires_grad=True),
              torch.tensor(np.asarray(w["%s/%s/b" % (name, c)], np.float64), requires_grad=True)) for c in convs}
    cur = torch.tensor(np.asarray(x, np.float64).reshape((B * T,) + x.shape[2:]))
    for c in convs:
        cur = conv_pool(cur, *ws[c]) if codes is None else routed_pool(cur, *ws[c], codes[c])
    feat_t = cur.reshape(B, T, -1)
    feat = feat_t.detach().numpy()
    wb = lambda p: (w[p + "/W"], w[p + "/U"], w[p + "/b"])
    caches, ys, h = [], [], feat
    for k in range(len(s["layers"])):
        p = "%s/l%d" % (name, k)
        h, cache = kr.bilstm_forward(h, wb(p + "/fwd"), wb(p + "/bwd"))
        caches.append(cache)
        ys.append(h)
    out = ys[0] + ys[1] if (s.get("residual") and len(ys) == 2) else ys[-1]
    P, hc = kr.dense_softmax_forward(out, None, w["dense/W"], w["dense/b"])
    loss_b, dz = kr.ctc_loss_grad(P, labels, input_length, label_length, skip=spec["ctc"]["skip"], eps=spec["ctc"]["eps"])
    grads = {}
    da, grads["dense/W"], grads["dense/b"] = kr.dense_backward(dz / B, hc)
    dy = da
    for k in range(len(s["layers"]) - 1, -1, -1):
        p = "%s/l%d" % (name, k)
        dx, gf, gb = kr.bilstm_backward(dy, caches[k], need_dx=True)
        for d, g in (("fwd", gf), ("bwd", gb)):
            grads[p + "/%s/W" % d], grads[p + "/%s/U" % d], grads[p + "/%s/b" % d] = g
        dy = dx + da if (k == 1 and s.get("residual")) else dx
    feat_t.backward(torch.tensor(dy))
    for c in convs:
        grads["%s/%s/W" % (name, c)] = ws[c][0].grad.numpy()
        grads["%s/%s/b" % (name, c)] = ws[c][1].grad.numpy()
    return float(loss_b.mean()), loss_b, grads, P
