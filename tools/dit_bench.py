"""DiT-XL/2 forward timing (BASELINE config C5 geometry: 4x32x32 latents, CFG batch 2 x 32) per GEMM math: 'fp32',
'fp16x2' (the default, fp32-accurate) and 'fp16' (DM_MATH_FP16, one fp16 product per MAC, no fp32 parity).

One model object (its own native handle and cached plan) per arithmetic, all in one process, timed in alternating
rounds so every arithmetic sees the same box state; the spread of an arithmetic is (max - min) / min over its rounds.
Then the per-launch times of the token GEMM kernels from each plan's own profile (events around every launch: not
an end-to-end figure).

    python tools/dit_bench.py [--batch 64] [--iters 5] [--rounds 5] [--math fp32 fp16x2 fp16] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'diffusion-models-pytorch_amd')]

import torch  # noqa: E402

import dmhip  # noqa: E402
from models.dit.model import DiT_models  # noqa: E402
from utils.synthetic import init_synthetic_  # noqa: E402

GFLOP = 237.2  # per image per forward (analytic)


def timed(model, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        model(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def profile(model, abi, args, iters=3):
    """{label: (launches per forward, us per launch)} of one profiled run, by total time."""
    h = model.native_handle(args[0].device)
    dmhip.unet_profile_enable(h, True, abi=abi)
    for _ in range(iters):
        model(*args)
    torch.cuda.synchronize()
    ops = dmhip.unet_profile_read(h, abi=abi)
    dmhip.unet_profile_enable(h, False, abi=abi)
    by = {}
    for op in ops:
        if op['launches']:
            e = by.setdefault(op['label'], [0, 0.0, []])
            e[0] += op['launches']
            e[1] += op['ms_total']
            e[2].append((op['flops'], op['ms_total'] / op['launches'] * 1e3))
    return by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--math', nargs='+', default=['fp32', 'fp16x2', 'fp16'], choices=sorted(dmhip.TOKEN_MATH))
    ap.add_argument('--json', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dit_bench: no GPU visible (a timing needs the device)')
    dev = torch.device('cuda', 0)
    B = args.batch
    g = torch.Generator().manual_seed(0)
    inp = (torch.randn((B, 4, 32, 32), generator=g).to(dev), torch.randint(0, 1000, (B, ), generator=g).to(dev),
           torch.randint(0, 1000, (B, ), generator=g).to(dev))
    models = {}
    for math in args.math:
        m = DiT_models['DiT-XL/2'](input_size=32, num_classes=1000, learn_sigma=True).eval()
        init_synthetic_(m)
        m.set_math(math)
        models[math] = m.to(dev)
        for _ in range(3):   # plan build, graph capture, warm-up
            models[math](*inp)
    torch.cuda.synchronize()
    res = {math: [] for math in models}
    for _ in range(args.rounds):
        for math, m in models.items():
            res[math].append(timed(m, inp, args.iters))
    out = dict(batch=B, iters=args.iters, rounds=args.rounds, device=torch.cuda.get_device_name(0), forward_ms=res)
    for math, v in res.items():
        ms = min(v)
        print(f'DiT-XL/2 B={B} {math:7s} {ms:8.2f} ms/forward (rounds ' + ' '.join(f'{x:.2f}' for x in v) +
              f'; spread {(max(v) - ms) / ms * 100:.1f} %)  {B * GFLOP / ms:7.1f} TFLOP/s  '
              f'{B / ms * 1e3:8.1f} img-forwards/s', flush=True)
    if 'fp16' in res and 'fp16x2' in res:
        out['fp16x2_over_fp16'] = min(res['fp16x2']) / min(res['fp16'])
        print(f'fp16x2 / fp16 = x{out["fp16x2_over_fp16"]:.3f}')
    out['profile'] = {}
    for math, m in models.items():
        if math == 'fp32':
            continue
        by = profile(m, 'dm_dit', inp)
        tot = sum(v[1] for v in by.values()) / 3
        print(f'{math}: {tot:.2f} ms per forward in kernels (profiled)')
        rows = {}
        for label, (n, ms, each) in sorted(by.items(), key=lambda kv: -kv[1][1])[:10]:
            print(f'  {label:36s} {n // 3:4d} launches/forward {ms / n * 1e3:9.1f} us each  {ms / 3:7.2f} ms/forward')
            rows[label] = dict(launches=n // 3, us_per_launch=ms / n * 1e3, ms_per_forward=ms / 3)
        # the token GEMMs by their FLOP count (qkv 3 D^2, proj D^2, fc1 / fc2 4 D^2 per token: fc1 before fc2)
        for label in ('linear_h16_kernel', 'linear_k32_kernel<3>'):
            if label in by:
                shapes = {}
                for fl, us in by[label][2]:
                    shapes.setdefault(round(fl / 1e9), []).append(us)
                for fl, us in sorted(shapes.items()):
                    mean = sum(us) / len(us)
                    # (ops of one FLOP count alternate in plan order: fc1, fc2, fc1, ...)
                    a, b = us[0::2], us[1::2]
                    alt = f'; alternating {sum(a) / len(a):.1f} / {sum(b) / len(b):.1f} us' if len(us) > 2 else ''
                    print(f'    {label} {fl:6d} GFLOP: {len(us):3d} ops, {mean:8.1f} us per launch '
                          f'({fl / mean * 1e3:7.1f} TFLOP/s){alt}')
                    rows[f'{label}@{fl}GF'] = dict(ops=len(us), us_per_launch=mean,
                                                   us_even_odd=[sum(a) / len(a), sum(b) / len(b)] if len(us) > 2 else None)
        out['profile'][math] = rows
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
