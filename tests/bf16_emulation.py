"""The yardstick of the bf16 encoder tests: a float64 (or float32) emulation of the bf16 conv stack written with
torch CPU ops only -- no call into the library.  Operands are rounded to bf16 with ``tensor.to(torch.bfloat16)``
(round to nearest even), products are accumulated by ``F.conv2d`` in ``acc`` precision, bias and LeakyReLU(0.05)
follow in ``acc`` precision, and a layer's output is rounded to bf16 wherever the HIP path rounds it."""

import torch
import torch.nn.functional as F

SLOPE = 0.05


def rne_bf16(t):
    """``t`` rounded to the nearest bf16 value (ties to even), returned in ``t``'s dtype.  fp32 goes through
    ``tensor.to(torch.bfloat16)``; float64 is rounded to 8 significant bits directly (through fp32 it would be
    rounded twice), normal range only."""
    if t.dtype != torch.float64:
        return t.to(torch.bfloat16).to(t.dtype)
    m, e = torch.frexp(t)                       # t = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def conv_layer(x, w, b, stride, pads, act=True, acc=torch.float64):
    """One layer: x (N,C,H,W), w (K,C,R,S), b (K) or None; pads = (left, right, top, bottom).  No rounding here."""
    h = F.pad(x.to(acc), pads)
    y = F.conv2d(h, w.to(acc), None if b is None else b.to(acc), stride=stride)
    return F.leaky_relu(y, SLOPE) if act else y


def pads_of(geom):
    """(left, right, top, bottom) zero padding implied by the twelve geometry integers of ConvLayerPlan.geom."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    pb = max((P - 1) * st + R - pt - H, 0)
    pr = max((Q - 1) * st + S - pl - W, 0)
    return (pl, pr, pt, pb)


def crop_to(y, geom):
    """F.conv2d on a map padded beyond what (P, Q) need yields extra rows / columns: keep the plan's."""
    return y[:, :, :geom[10], :geom[11]]


def stack_features(layers, x, acc=torch.float64):
    """The whole stack.  layers = [(w fp32, b fp32, stride, pads)], x fp32 frames in [0, 1] (N,C,H,W).
    Layer 1 is fp32 arithmetic on the device (operands NOT rounded); layers 2.. multiply bf16 operands; every
    layer but the last rounds its output to bf16.  -> (N, C*H*W) in ``acc``."""
    h = x
    last = len(layers) - 1
    for i, (w, b, stride, pads) in enumerate(layers):
        if i > 0:
            w = rne_bf16(w.float())
        h = conv_layer(h, w, b, stride, pads, True, acc)
        if i < last:
            h = rne_bf16(h)
    return h.reshape(h.shape[0], -1)


def oracle_layers(enc):
    """[(w, b, stride, pads)] of an oracle ``ConvEncoder`` (oracle/ref_cpu.py) without pooling / batch norm."""
    out = []
    for name, pad, bn, pool in enc.layers:
        assert bn is None and pool is None
        conv = getattr(enc.encoder, name)
        if pad is None:
            py, px = conv.padding
            pad = (px, px, py, py)
        out.append((conv.weight.detach().float(), conv.bias.detach().float(), conv.stride[0], tuple(pad)))
    return out
