"""The LSUN-Church 256^2 DDPM UNet (configs/pesser_lsun_church_256.yaml, synthetic weights): forward time with the
C = 512 attention blocks on the fused L = 256 core (the default) against the three-launch path (DM_ATTN=unfused), the
two plans alternating in one process in both orders, plus the attention blocks' share of the forward and the
per-launch time of the 512 kernel against the launches it replaces, from the plans' own per-launch profiles
(dm_unet_profile).

    python tools/pesser_bench.py [--batch 8] [--iters 5] [--rounds 3] [--attn fused] [--json out.json]

--attn MODE times DM_ATTN=MODE (fused: attn_fused_kernel<512> on fp32 q | k | v rows; noproj / presplit) in place of
the default plan; DM_HIP_LIB selects another library build (tools/alt_lib.sh) for A/Bs of kernel variants.
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

CONFIG = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs', 'pesser_lsun_church_256.yaml')


def timed(model, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        model(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def profile(model, args, iters):
    """The plan's ops in launch order with ms per launch (events around every launch: not an end-to-end figure)."""
    h = model.native_handle(args[0].device)
    dmhip.unet_profile_enable(h, True)
    for _ in range(iters):
        model(*args)
    torch.cuda.synchronize()
    ops = dmhip.unet_profile_read(h)
    dmhip.unet_profile_enable(h, False)
    return [dict(label=op['label'], ms=op['ms_total'] / max(op['launches'], 1)) for op in ops]


def attention_spans(ops):
    """Index ranges [first, last] of the launches of each unfolded attention block: from the gn_partial / gn_finalize
    ahead of its qkv projection to its output projection. A block is recognised by its core: the fused kernel, or
    softmax_rows between the S and PV GEMMs."""
    spans = []
    for i, op in enumerate(ops):
        if not (op['label'].startswith(('attn_presplit_kernel', 'attn_fused_kernel')) or op['label'] == 'softmax_rows'):
            continue
        core_first = i - 1 if op['label'] == 'softmax_rows' else i
        core_last = i + 1 if op['label'] == 'softmax_rows' else i
        first = core_first
        while first > 0 and not ops[first - 1]['label'].startswith(('gn_finalize', 'gn_partial')):
            first -= 1   # back over the qkv projection (and linear_presplit_a) to the block's GroupNorm launches
        while first > 0 and ops[first - 1]['label'].startswith(('gn_finalize', 'gn_partial')):
            first -= 1
        last = core_last if ops[core_last]['label'].endswith(',proj>') else core_last + 1
        spans.append(dict(first=first, last=last, core_first=core_first, core_last=core_last))
    return spans


def summarise(ops):
    spans = attention_spans(ops)
    total = sum(op['ms'] for op in ops)
    blocks = [sum(op['ms'] for op in ops[s['first']:s['last'] + 1]) for s in spans]
    cores = [sum(op['ms'] for op in ops[s['core_first']:s['core_last'] + 1]) for s in spans]
    return dict(kernel_ms=total, attention_blocks=len(spans), attention_ms=sum(blocks),
                attention_share=sum(blocks) / total if total else 0.0, core_ms_each=cores,
                core_labels=[[op['label'] for op in ops[s['core_first']:s['core_last'] + 1]] for s in spans])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--attn', type=str, default=None, help='DM_ATTN mode of the second arm (default: unset)')
    ap.add_argument('--json', type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pesser_bench: no GPU visible (a timing needs the device)')
    dev = torch.device('cuda', 0)
    conf = load_config(CONFIG)
    g = torch.Generator().manual_seed(0)
    args = (torch.randn((a.batch, 3, 256, 256), generator=g).to(dev),
            torch.randint(0, 1000, (a.batch, ), generator=g).to(dev))
    # DM_ATTN is read when a plan is built: one model per arm, each building its plan under its own setting
    models = {}
    saved = os.environ.get('DM_ATTN')
    for arm, mode in (('unfused', 'unfused'), ('default', a.attn)):
        if mode is None:
            os.environ.pop('DM_ATTN', None)
        else:
            os.environ['DM_ATTN'] = mode
        m = instantiate_from_config(conf.model).eval()
        init_synthetic_(m)
        models[arm] = m.to(dev)
        for _ in range(3):   # plan build, graph capture, warm-up
            models[arm](*args)
        torch.cuda.synchronize()
    if saved is None:
        os.environ.pop('DM_ATTN', None)
    else:
        os.environ['DM_ATTN'] = saved
    same = torch.equal(models['unfused'](*args), models['default'](*args))
    res = {arm: [] for arm in models}
    for order in (('unfused', 'default'), ('default', 'unfused')):   # both orders, so neither arm always runs warm
        for _ in range(a.rounds):
            for arm in order:
                res[arm].append(timed(models[arm], args, a.iters))
    out = dict(batch=a.batch, iters=a.iters, rounds=a.rounds, second_arm=a.attn or 'default', library=dmhip.lib_path,
               device=torch.cuda.get_device_name(0), forward_ms=res, outputs_bit_identical=same)
    n = a.rounds
    for arm, v in res.items():
        print(f'{arm:8s} B={a.batch}: ' + ' '.join(f'{x:.2f}' for x in v) + f' ms/forward (min {min(v):.2f})',
              flush=True)
    for k, sl in (('unfused_first', slice(0, n)), ('default_first', slice(n, 2 * n))):
        r = min(res['default'][sl]) / min(res['unfused'][sl])
        out[f'default_over_unfused_{k}'] = r
        print(f'default / unfused, {k.replace("_", " ")}: {r:.4f}')
    print(f'second arm: DM_ATTN={a.attn or "(unset)"}; outputs bit-identical: {same}')
    for arm, m in models.items():
        ops = profile(m, args, 3)
        s = summarise(ops)
        out[f'profile_{arm}'] = s
        by = {}
        for op in ops:
            e = by.setdefault(op['label'], [0.0, 0])
            e[0] += op['ms']
            e[1] += 1
        out[f'ops_{arm}'] = {k: dict(ms_per_forward=v[0], launches=v[1]) for k, v in by.items()}
        print(f'{arm}: {s["kernel_ms"]:.2f} ms per forward in kernels; {s["attention_blocks"]} unfolded attention '
              f'blocks {s["attention_ms"]:.3f} ms = {100 * s["attention_share"]:.2f} %')
        for labels, ms in zip(s['core_labels'], s['core_ms_each']):
            print(f'  core {" + ".join(labels):70s} {ms * 1e3:9.1f} us')
        for label, v in sorted(by.items(), key=lambda kv: -kv[1][0])[:10]:
            print(f'  {label:60s} {v[1]:4d} launches/forward {v[0]:8.3f} ms')
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
