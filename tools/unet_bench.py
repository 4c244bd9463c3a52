"""Forward timing of the conv denoisers in the default 'fp16x2' arithmetic and with the conv-half option
(dm_unet_set_conv_half: one fp16 product per MAC in the covered 3x3 convs, no fp32 parity):

    cifar    the CIFAR-10 UNet (configs/ddpm_cifar10.yaml) at B = 256, 32 x 32
    adm256   the conditional half of ADM-256 (configs/adm256_combined.yaml) at --adm_batch (default 8), 256 x 256
    pesser   the LSUN-Church DDPM UNet (configs/pesser_lsun_church_256.yaml) at B = 8, 256 x 256

One model object (its own native handle and cached plan) per arithmetic, both in one process, timed in alternating
rounds so both see the same box state; the figure is the minimum over the rounds and the spread (max - min) / min.
Then the per-launch times of the 3x3 conv kernels from each plan's own profile (events around every launch: not an
end-to-end figure), grouped by map size: what conv_h16_kernel and its image pass cost against the kernels they replace.

--ab_lib PATH (e.g. tools/lib/libprev.so, the parent commit's library from tools/build_prev.sh, run before this
change is committed) adds the "did fp16x2 move" arm: --ab_runs child processes per library, alternating PATH (through
DM_HIP_LIB) and this build, each timing the fp16x2 forward alone (--only fp16x2); per config the minimum and the
spread over all of a library's rounds.

    python tools/unet_bench.py [--configs cifar adm256 pesser] [--iters 5] [--rounds 5] [--only fp16x2]
                               [--ab_lib tools/lib/libprev.so] [--ab_runs 2] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'diffusion-models-pytorch_amd')]

import torch  # noqa: E402

import dmhip  # noqa: E402
from utils.misc import instantiate_from_config, load_config  # noqa: E402
from utils.synthetic import init_synthetic_  # noqa: E402

CFG = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs')
KINDS = ['fp16x2', 'conv_half']
CONV3 = ('conv_wino', 'conv_k32', 'conv_patch3', 'conv_h16_kernel')


def build(name, dev, adm_batch):
    """-> (make(): a fresh model on the device, inputs)"""
    g = torch.Generator().manual_seed(0)
    if name == 'cifar':
        conf, B, S, C = load_config(os.path.join(CFG, 'ddpm_cifar10.yaml')), 256, 32, 3
        make = lambda: instantiate_from_config(conf.model).eval()   # noqa: E731
        y = None
    elif name == 'adm256':
        conf, B, S, C = load_config(os.path.join(CFG, 'adm256_combined.yaml')), adm_batch, 256, 3
        make = lambda: instantiate_from_config(conf.model).eval().unet_cond   # noqa: E731
        y = torch.randint(0, 1000, (B, ), generator=g).to(dev)
    else:
        conf, B, S, C = load_config(os.path.join(CFG, 'pesser_lsun_church_256.yaml')), 8, 256, 3
        make = lambda: instantiate_from_config(conf.model).eval()   # noqa: E731
        y = None
    x = torch.randn((B, C, S, S), generator=g).to(dev)
    t = torch.randint(0, 1000, (B, ), generator=g).to(dev)
    return make, (x, t) if y is None else (x, t, y)


def timed(model, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        model(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def profile(model, args, iters=3):
    """The plan's ops in launch order: label, flops, bytes, us per launch."""
    h = model.native_handle(args[0].device)
    dmhip.unet_profile_enable(h, True)
    for _ in range(iters):
        model(*args)
    torch.cuda.synchronize()
    ops = dmhip.unet_profile_read(h)
    dmhip.unet_profile_enable(h, False)
    return [dict(label=op['label'], flops=op['flops'], bytes=op['bytes'],
                 us=op['ms_total'] / max(op['launches'], 1) * 1e3) for op in ops]


def conv_rows(ops):
    """{GFLOP of a 3x3 conv (its shape's signature): [us of the conv, us of the image pass ahead of it]} per op."""
    rows = {}
    for i, op in enumerate(ops):
        if not op['label'].startswith(CONV3) or op['flops'] <= 0:
            continue
        img = ops[i - 1]['us'] if i and ops[i - 1]['label'] == 'conv_h16_image' else 0.0
        rows.setdefault(round(op['flops'] / 1e9, 2), []).append((op['label'].split('<')[0], op['us'], img))
    return rows


def ab_libs(args):
    """fp16x2 forwards of --ab_lib and of this build in alternating child processes -> {config: {lib: [ms]}}."""
    import subprocess
    import tempfile
    res = {}
    for run in range(args.ab_runs):
        for tag, lib in (('other', os.path.abspath(args.ab_lib)), ('this', None)):
            env = dict(os.environ)
            env.pop('DM_HIP_LIB', None)
            if lib:
                env['DM_HIP_LIB'] = lib
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, 'ab.json')
                subprocess.run([sys.executable, os.path.abspath(__file__), '--only', 'fp16x2', '--configs', *args.configs,
                                '--adm_batch', str(args.adm_batch), '--iters', str(args.iters), '--rounds',
                                str(args.rounds), '--json', out], env=env, check=True, stdout=subprocess.DEVNULL)
                with open(out) as f:
                    got = json.load(f)
            for name, row in got['configs'].items():
                res.setdefault(name, {}).setdefault(tag, []).extend(row['forward_ms']['fp16x2'])
    for name, by in res.items():
        for tag, v in by.items():
            print(f'{name} fp16x2 {tag:5s} library: {min(v):9.2f} ms/forward over {len(v)} rounds in {args.ab_runs} '
                  f'processes (spread {(max(v) - min(v)) / min(v) * 100:.1f} %)', flush=True)
        print(f'{name}: this / other = {min(by["this"]) / min(by["other"]):.4f}', flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['cifar', 'adm256', 'pesser'], choices=['cifar', 'adm256', 'pesser'])
    ap.add_argument('--adm_batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', type=str, default=None, choices=KINDS)
    ap.add_argument('--json', type=str, default=None)
    ap.add_argument('--ab_lib', type=str, default=None, help='another library build to time fp16x2 against')
    ap.add_argument('--ab_runs', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('unet_bench: no GPU visible (a timing needs the device)')
    dev = torch.device('cuda', 0)
    kinds = [args.only] if args.only else KINDS
    out = dict(device=torch.cuda.get_device_name(0), lib=os.environ.get('DM_HIP_LIB', ''), iters=args.iters,
               rounds=args.rounds, configs={})
    for name in args.configs:
        make, inp = build(name, dev, args.adm_batch)
        models = {}
        for kind in kinds:
            m = make()
            init_synthetic_(m)
            if kind == 'conv_half':   # (the fp16x2 arm never touches the switch: it also runs on an older library)
                m.set_conv_half(True)
            models[kind] = m.to(dev)
            for _ in range(3):   # plan build, graph capture, warm-up
                models[kind](*inp)
        torch.cuda.synchronize()
        res = {k: [] for k in models}
        for _ in range(args.rounds):
            for k, m in models.items():
                res[k].append(timed(m, inp, args.iters))
        B = inp[0].shape[0]
        row = dict(batch=B, forward_ms=res)
        for k, v in res.items():
            ms = min(v)
            print(f'{name} B={B} {k:9s} {ms:9.2f} ms/forward (rounds ' + ' '.join(f'{x:.2f}' for x in v) +
                  f'; spread {(max(v) - ms) / ms * 100:.1f} %)  {B / ms * 1e3:8.1f} img-forwards/s', flush=True)
        if len(res) == 2:
            row['fp16x2_over_conv_half'] = min(res['fp16x2']) / min(res['conv_half'])
            print(f'{name}: fp16x2 / conv_half = x{row["fp16x2_over_conv_half"]:.3f}')
        row['profile'] = {}
        for k, m in models.items():
            ops = profile(m, inp)
            tot = sum(op['us'] for op in ops) / 1e3
            conv = sum(op['us'] for op in ops if op['label'].startswith(CONV3)) / 1e3
            img = sum(op['us'] for op in ops if op['label'] == 'conv_h16_image') / 1e3
            print(f'  {k}: {tot:.2f} ms per forward in kernels (profiled), 3x3 conv kernels {conv:.2f} ms, '
                  f'image passes {img:.2f} ms')
            rows = conv_rows(ops)
            for gf, each in sorted(rows.items()):
                labels = sorted({e[0] for e in each})
                us = sum(e[1] for e in each) / len(each)
                im = sum(e[2] for e in each) / len(each)
                print(f'    {gf:9.2f} GFLOP x {len(each):3d}: {us:9.1f} us per launch'
                      + (f' + {im:7.1f} us image' if im else '') + f' ({gf / (us + im) * 1e3:7.1f} TFLOP/s)  {",".join(labels)}')
            row['profile'][k] = dict(kernel_ms=tot, conv3_ms=conv, image_ms=img,
                                     convs={str(gf): dict(n=len(e), us=sum(x[1] for x in e) / len(e),
                                                          image_us=sum(x[2] for x in e) / len(e),
                                                          labels=sorted({x[0] for x in e})) for gf, e in rows.items()})
        out['configs'][name] = row
        del models
        torch.cuda.empty_cache()
    if args.ab_lib:
        out['ab_fp16x2_ms'] = ab_libs(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
