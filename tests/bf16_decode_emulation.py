"""The yardstick of the bf16 decoder tests: a float64 (or float32) emulation of the bf16 transposed-conv stack written
with torch CPU ops only -- no call into the library.  A layer is ``F.conv_transpose2d`` without padding (the
full-size map) in ``acc`` precision, then the plan's crop (output pixel o is full-size pixel o + crop; pixels past
the full size, which 'valid' padding reaches through output_padding, are zero), bias and activation in ``acc``
precision.  Operands and outputs are rounded to bf16 (``tests.bf16_emulation.rne_bf16``) exactly where the HIP path
rounds: the stack's input, the weights of every body layer, the output of every body layer but the stack's last.
A last layer of 1..4 channels -- the layer onto the frame -- multiplies its UNROUNDED fp32 weights and keeps its output."""

import torch
import torch.nn.functional as F

from tests.bf16_emulation import SLOPE, rne_bf16

ACT_NONE, ACT_LRELU, ACT_SIGMOID = 0, 1, 2


def convT_layer(x, w, b, geom, act, acc=torch.float64):
    """One layer: x (N,Ci,Hi,Wi), w (Ci,Co,R,S), b (Co) or None, geom the twelve integers of ConvLayerPlan.geom
    (N, Ci, Hi, Wi, Co, R, S, stride, crop_t, crop_l, Ho, Wo).  No rounding here."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    full = F.conv_transpose2d(x.to(acc), w.to(acc), None, stride=st)
    y = torch.zeros((x.shape[0], Co, Ho, Wo), dtype=acc)
    h = min(Ho, full.shape[2] - ct)
    v = min(Wo, full.shape[3] - cl)
    y[:, :, :h, :v] = full[:, :, ct:ct + h, cl:cl + v]
    if b is not None:
        y = y + b.to(acc).view(1, -1, 1, 1)
    if act == ACT_LRELU:
        return F.leaky_relu(y, SLOPE)
    if act == ACT_SIGMOID:
        return torch.sigmoid(y)
    return y


def is_frame_layer(i, layers):
    """The stack's last layer runs on the vector unit with fp32 weights iff it has 1..4 output channels."""
    return i == len(layers) - 1 and layers[i][0].shape[1] <= 4


def stack_output(layers, h, acc=torch.float64):
    """The whole stack.  layers = [(w fp32 (Ci,Co,R,S), b fp32, geom, act)], h the fp32 (or float64) stack input
    (N,C,H,W) -- the dense layer's output.  -> (N, Co, Ho, Wo) in ``acc``."""
    a = rne_bf16(h.to(acc))
    last = len(layers) - 1
    for i, (w, b, geom, act) in enumerate(layers):
        geom = (a.shape[0],) + tuple(geom[1:])
        if is_frame_layer(i, layers):
            a = convT_layer(a, w.float(), b, geom, act, acc)
        else:
            a = convT_layer(a, rne_bf16(w.float()), b, geom, act, acc)
            if i < last:
                a = rne_bf16(a)
    return a


def plan_layers(decoder, dataset=None, gain=1.0):
    """[(w, b, geom, act)] on the CPU from a ``ConvAEDecoder``'s plan and parameters (weights times ``gain``)."""
    params = decoder._stack_params(dataset)
    return [(params[2 * i].detach().float().cpu() * gain, params[2 * i + 1].detach().float().cpu(), layer.geom(1),
             layer.act) for i, layer in enumerate(decoder._plan)]
