"""fp32 against bf16 decoding (hparams['hip_decode_dtype']) from device-resident latents, alternated in ONE process.

Per shape: every (shape, dtype) is warmed first, then fp32 and bf16 windows of at least --window seconds alternate
--reps times with a device synchronise around each window.  Three blocks per shape:

* ``get_reconstruction`` from latents end to end (it ends in a copy of the frames to the host, the same bytes in
  both arithmetics) and the decoder on the device alone (``model.decoding`` inside ``decode_precision``): ms per
  trial and frames/s for both dtypes (median, with the spread over the windows), the ratio, max |dx_hat| / max |x_hat|;
* every layer on its own, hipEvents around --layer-iters back-to-back launches on the layer's real operands: the
  fp32 entry point against the bf16 one, GFLOP and the share of the 2.5 PFLOP/s bf16 matrix peak, then the two
  helpers only the bf16 stack has (weight pack, stack input).
    python tools/bench_decode.py [--reps 5] [--window 1.0] [--layer-iters 50]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting.eval import get_reconstruction
from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from behavenet_amd.data.synthetic import base_hparams

BF16_PEAK = 2.5e15
SHAPES = [('256x1x128x128', 256, [1, 128, 128]),
          ('189x2x128x128', 189, [2, 128, 128]),
          ('256x1x64x48', 256, [1, 64, 48])]


def build(dim):
    arch = load_handcrafted_arch(list(dim), 12, None, check_memory=False)
    torch.manual_seed(0)
    return AE(base_hparams(arch, 'ae', {'device': 'cuda'})).to('cuda').eval()


def window(fn, trials, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        for t in trials:
            fn(t)
        n += len(trials)
        if n % (4 * len(trials)) == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def alternate(name, what, n, fns, trials, reps, seconds):
    ms = {'f32': [], 'bf16': []}
    for _ in range(reps):
        for dtype in ('f32', 'bf16'):
            ms[dtype].append(window(fns[dtype], trials, seconds))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in ('f32', 'bf16'):
        print('%-14s %-28s %-4s %.4f ms per trial (min %.4f max %.4f over %d windows), %.0f frames/s'
              % (name, what, k, med[k], min(ms[k]), max(ms[k]), reps, n / med[k] * 1e3))
    print('%-14s %-28s f32 / bf16 = %.2f (slowest bf16 window against fastest f32 window: %.2f)'
          % (name, what, med['f32'] / med['bf16'], min(ms['f32']) / max(ms['bf16'])))


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(5):
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        best.append(a.elapsed_time(b) / iters)
    return statistics.median(best)


def per_layer(name, model, z, iters):
    dec = model.decoding
    plan, params = dec._plan, [p.detach() for p in dec._stack_params(None)]
    n = z.shape[0]
    start = dec.hparams['ae_decoding_starting_dim']
    with torch.no_grad():
        h32 = hf.linear(z, dec.FF.weight, dec.FF.bias).view(n, start[0], start[1], start[2]).contiguous()
        a16 = _hip.to_nhwc_bf16(h32)
        last = len(plan) - 1
        tot = {'f32': 0.0, 'bf16': 0.0}
        for i, layer in enumerate(plan):
            w, b, g = params[2 * i], params[2 * i + 1], layer.geom(n)
            # multiply-adds that reach an output pixel: every input pixel meets every tap once
            gflop = 2.0 * n * layer.cin * layer.hin * layer.win * layer.cout * layer.R * layer.S / 1e9
            t32 = event_ms(lambda: hf._fwd(layer, h32, w, b), iters)
            if i == last and layer.cout <= 4:
                t16 = event_ms(lambda: _hip.convT2d_last_bf16(a16, w, b, g, layer.act, hf.LRELU_SLOPE), iters)
                nxt = None
            else:
                wp = _hip.convT_pack_w_bf16(w, torch.empty(_hip.convT_pack_w_bf16_bytes(w.shape), dtype=torch.uint8,
                                                           device='cuda'))
                t16 = event_ms(lambda: _hip.convT2d_fwd_bf16(a16, wp, b, g, layer.act, hf.LRELU_SLOPE, i == last), iters)
                nxt = _hip.convT2d_fwd_bf16(a16, wp, b, g, layer.act, hf.LRELU_SLOPE, False)
            tot['f32'] += t32
            tot['bf16'] += t16
            print('%-14s convT%d %-44r f32 %7.1f us  bf16 %7.1f us  f32 / bf16 = %.2f  %6.2f GFLOP  %.3f of the bf16 peak'
                  % (name, i, layer, t32 * 1e3, t16 * 1e3, t32 / t16, gflop, gflop * 1e9 / (t16 * 1e-3) / BF16_PEAK))
            h32 = hf._fwd(layer, h32, w, b)
            a16 = nxt
        body = [i for i in range(len(plan)) if not (i == last and plan[i].cout <= 4)]
        bufs = [torch.empty(_hip.convT_pack_w_bf16_bytes(params[2 * i].shape), dtype=torch.uint8, device='cuda')
                for i in body]
        t_pack = event_ms(lambda: [_hip.convT_pack_w_bf16(params[2 * i], buf) for i, buf in zip(body, bufs)], iters)
        h0 = hf.linear(z, dec.FF.weight, dec.FF.bias).view(n, start[0], start[1], start[2]).contiguous()
        t_in = event_ms(lambda: _hip.to_nhwc_bf16(h0), iters)
        t_ff = event_ms(lambda: hf.linear(z, dec.FF.weight, dec.FF.bias), iters)
    print('%-14s layers summed: f32 %.1f us, bf16 %.1f us; bf16 only: weight pack (%d layers) %.1f us, stack input '
          '%.1f us; both: FF %.1f us' % (name, tot['f32'] * 1e3, tot['bf16'] * 1e3, len(body), t_pack * 1e3,
                                         t_in * 1e3, t_ff * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--layer-iters', type=int, default=50)
    args = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for name, n, dim in SHAPES:
        model = build(dim)
        g = torch.Generator().manual_seed(1)
        trials = [torch.randn((n, model.decoding.FF.in_features), generator=g).to('cuda') for _ in range(8)]

        def recon(dtype):
            def run(z):
                model.hparams['hip_decode_dtype'] = dtype
                return get_reconstruction(model, z)
            return run

        def device_only(dtype):
            def run(z):
                with torch.no_grad(), hf.decode_precision(dtype):
                    return model.decoding(z, None, None, dataset=None)
            return run
        x = {}
        for dtype in ('f32', 'bf16'):                       # warm every shape in both arithmetics
            for t in trials:
                x[dtype] = recon(dtype)(t)
                device_only(dtype)(t)
        torch.cuda.synchronize()
        err = float(abs(x['bf16'] - x['f32']).max() / abs(x['f32']).max())
        alternate(name, 'get_reconstruction(latents)', n, {k: recon(k) for k in ('f32', 'bf16')}, trials, args.reps,
                  args.window)
        alternate(name, 'decoder on the device', n, {k: device_only(k) for k in ('f32', 'bf16')}, trials, args.reps,
                  args.window)
        print('%-14s max|x_bf16 - x_f32| / max|x_f32| = %.2e (freshly initialised weights)' % (name, err))
        per_layer(name, model, trials[0], args.layer_iters)


if __name__ == '__main__':
    main()
