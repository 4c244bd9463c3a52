"""The conv dispatch fixture (tests/golden/conv_dispatch.json): the enumeration of conv descriptors its generator
records (tests/golden/make_golden_conv_dispatch.py), how one row is asked of the library (dm_debug_conv_choice: host
only, stand-in addresses, no GPU), and which kernel name a `launched` answer ("family:variant")
must carry in its profile label.

A row is (shape, options, toggles), and the rows are enumerate_rows() in its order, so the fixture stores the answers
alone: the table of distinct answers [launched, label, emits_gn, lds_tables, drift] (about 200), one byte per row that
indexes it (zlib, base64), and the sha256 of the enumeration the bytes belong to.
"""
import base64
import hashlib
import itertools
import json
import os
import re
import zlib

SHAPE_KEYS = ('taps', 'stride', 'upsample', 's2_pad0', 'Hin', 'Win', 'Cin1', 'Cin2', 'Cout', 'B')
# weights: 0 none, 1 bf16x3, 2 fp16x2, 3 fp16x2 + w_wino (fold 0), 4 fp16x2 + w_wino (fold 1); with upsample = 2 the
# library reads w_wino as the sub-pixel Winograd image. pro: 0 none, 1 pro_scale tables, 2 the in-kernel finalize (gin).
# bad: 0 a well-formed descriptor; else one defect (BAD below).
OPT_KEYS = ('weights', 'tile', 'h16', 'pro', 'nosilu', 'ksplit', 'gn_G', 'gn_emit', 'res', 'rowvec', 'pitch_extra',
            'misalign_y', 'pick_B', 'bad')
OPT_DEFAULT = dict(weights=2, tile=0, h16=0, pro=0, nosilu=0, ksplit=1, gn_G=0, gn_emit=0, res=0, rowvec=0,
                   pitch_extra=0, misalign_y=0, pick_B=256, bad=0)
BAD = {1: 'K mismatch', 2: 'output one row short', 3: 'x_pitch not a multiple of 4', 4: 'w_wino without w_split',
       5: 'misaligned w', 6: 'y_pitch below Cout', 7: 'split-K without a workspace'}

# every dispatch toggle at its default (no variable set) and flipped, one at a time
TOGGLE_ENV = ('DM_CONV_WINO', 'DM_CONV_SUBWINO', 'DM_CONV_K32S', 'DM_CONV_K32S2', 'DM_CONV_K32T2', 'DM_K32_8X',
              'DM_K32S_W4', 'DM_GN_FUSION')
TOGGLES = [{}] + [{n: ('1' if n == 'DM_K32S_W4' else '0')} for n in TOGGLE_ENV]

SQUARE = [(n, n) for n in (4, 8, 16, 32, 64, 128, 256)]
AWKWARD = [(8, 16), (16, 8), (6, 6), (12, 12), (20, 20), (32, 64)]
MAPS = SQUARE + AWKWARD
# taps, stride, upsample, s2_pad0: every valid combination ...
GEOMS = [(9, 1, 0, 0), (9, 1, 1, 0), (9, 1, 2, 0), (9, 2, 0, 0), (9, 2, 0, 1), (1, 1, 0, 0)]
# ... and a few invalid ones
BAD_GEOMS = [(3, 1, 0, 0), (9, 3, 0, 0), (9, 2, 1, 0), (9, 1, 3, 0), (1, 2, 0, 0), (9, 1, 0, 1), (1, 1, 0, 1),
             (1, 1, 1, 0)]
CIN1 = (32, 64, 128, 256, 384, 512)
COUT = (32, 64, 128, 256, 512, 66)  # 66: not a multiple of 4


def shape(geom, hw, cin1, cin2, cout, B=2):
    return geom + hw + (cin1, cin2, cout, B)


def opt(**kw):
    d = dict(OPT_DEFAULT)
    d.update(kw)
    return tuple(d[k] for k in OPT_KEYS)


def enumerate_rows():
    """The fixture's rows: (shape tuple, options tuple, toggle index), in a fixed order, without repeats."""
    rows, seen = [], set()

    def add(s, o, t=0):
        key = (s, o, t)
        if key not in seen:
            seen.add(key)
            rows.append(key)

    # A. the shape axes in full: geometry x map x Cin1 x Cout x weights
    for g, hw, ci, co, w in itertools.product(GEOMS, MAPS, CIN1, COUT, (0, 2, 3)):
        add(shape(g, hw, ci, 0, co), opt(weights=w))
    for g, hw, ci, co in itertools.product(GEOMS, MAPS, (64, 384), (128, 66)):
        add(shape(g, hw, ci, 0, co), opt(weights=1))
    # B. prologue x statistics
    # -4: Cout / 4 groups; -2: Cout / 2, groups of two channels, which the direct kernels' epilogues emit and the
    # Winograd epilogue does not (the automatic choice then falls back to the direct kernels)
    gn = [(0, 0), (32, 1), (8, 1), (-4, 1), (32, 0), (-2, 1)]
    for g, hw, ci, co, w, pro, (G, emit) in itertools.product(GEOMS, SQUARE[:5] + [(8, 16)], (64, 512), (128, 512),
                                                               (2, 3), (0, 1, 2), gn):
        add(shape(g, hw, ci, 0, co), opt(weights=w, pro=pro, gn_G=co // -G if G < 0 else G, gn_emit=emit))
    for g, hw, w, (G, emit) in itertools.product(GEOMS, SQUARE[:5], (0, 1), gn[1:5]):
        add(shape(g, hw, 64, 0, 128), opt(weights=w, pro=1, nosilu=1, gn_G=32 if G < 0 else G, gn_emit=emit))
    # C. the shortcut segment, split-K, residual / row vector
    for g, hw, ci, c2, co, w, ks, emit in itertools.product((GEOMS[0], GEOMS[5], GEOMS[3]), SQUARE[:5], (128, 512),
                                                            (0, 64, 128), (128, 256), (1, 2, 3, 4), (1, 2, 4), (0, 1)):
        add(shape(g, hw, ci, c2, co), opt(weights=w, ksplit=ks, pro=emit, gn_G=32 * emit, gn_emit=emit, res=emit,
                                          rowvec=1 - emit))
    for g, hw, c2 in itertools.product(GEOMS, SQUARE[:4], (64, 128)):
        add(shape(g, hw, 128, c2, 128), opt(weights=3, res=1, rowvec=1))
        add(shape(g, hw, 128, c2, 128), opt(weights=0))
    # D. every forced tile (and 24, which is none)
    for t, g, hw, (ci, co), w in itertools.product(range(25), GEOMS, SQUARE, ((64, 128), (256, 256)), (0, 2, 3)):
        add(shape(g, hw, ci, 0, co), opt(weights=w, tile=t))
    for t, hw, ks, pro in itertools.product(range(25), SQUARE[:4], (2, 4), (0, 1)):
        add(shape(GEOMS[0], hw, 256, 0, 256), opt(weights=3, tile=t, ksplit=ks, pro=pro))
        add(shape(GEOMS[0], hw, 512, 0, 128), opt(weights=2, tile=t, pro=1, gn_G=32, gn_emit=1))
        add(shape(GEOMS[0], hw, 128, 0, 128), opt(weights=1, tile=t, ksplit=ks))
    # E. the conv-half mark
    for hw, ci, c2, co, t, emit, pro in itertools.product(MAPS, (32, 128, 512), (0, 64), (32, 128, 66), (0, 1, 2),
                                                          (0, 1), (0, 1)):
        add(shape(GEOMS[0], hw, ci, c2, co), opt(h16=1, tile=t, gn_G=32 * emit, gn_emit=emit, pro=pro))
    for g, hw in itertools.product(GEOMS, SQUARE[:5]):
        add(shape(g, hw, 64, 0, 128), opt(h16=1, weights=3))
        add(shape(g, hw, 64, 0, 128), opt(h16=1, weights=0))
    # F. the batch and the nominal batch of the heuristics
    for B, pb, g, hw, (ci, co), w in itertools.product((1, 2, 256), (0, 256), GEOMS, SQUARE[:5] + [(12, 12)],
                                                      ((64, 64), (128, 128), (256, 512)), (0, 2, 3)):
        add(shape(g, hw, ci, 0, co, B), opt(weights=w, pick_B=pb))
    # G. each toggle flipped
    for t, g, hw, (ci, co), w, ks, emit in itertools.product(range(1, len(TOGGLES)), GEOMS, SQUARE[:6],
                                                            ((128, 128), (512, 256)), (2, 3), (1, 2), (0, 1)):
        if ks == 1 or g == GEOMS[0]:
            add(shape(g, hw, ci, 0, co), opt(weights=w, ksplit=ks, gn_G=32 * emit, gn_emit=emit, pro=emit), t)
    # H. the concat pitch, a misaligned y, malformed descriptors
    for g, hw, (ci, co), w in itertools.product(GEOMS, SQUARE[:6] + AWKWARD[:2], ((64, 64), (256, 128)), (0, 2, 3)):
        add(shape(g, hw, ci, 0, co), opt(weights=w, pitch_extra=128))
        add(shape(g, hw, ci, 0, co), opt(weights=w, misalign_y=1))
        for bad in BAD:
            add(shape(g, hw, ci, 0, co), opt(weights=w, bad=bad, ksplit=2 if bad == 7 else 1))
    for g, hw, ci, w in itertools.product(BAD_GEOMS, SQUARE[1:4], (64, 48), (0, 2, 3)):
        add(shape(g, hw, ci, 0, 128), opt(weights=w))
    for g, hw in itertools.product(GEOMS, SQUARE[1:4]):
        add(shape(g, hw, 48, 0, 128), opt())   # Cin1 not a multiple of 32
        add(shape(g, hw, 64, 48, 128), opt())  # nor Cin2
    # I. forms the axes above do not reach: GroupNorm tables of 1024 channels for two 8 x 8 images (conv_k32's
    # big-table tiles), a 192-wide map (64-pixel row segments where the 128-pixel ones do not divide it)
    for hw, co, pro, emit in itertools.product(((8, 8), (16, 16)), (128, 512), (0, 1), (0, 1)):
        add(shape(GEOMS[0], hw, 1024, 0, co), opt(pro=pro, gn_G=32 * emit, gn_emit=emit))
    for t, ci, pro in itertools.product((0, 1 + TOGGLE_ENV.index('DM_CONV_K32T2')), (64, 256), (0, 1)):
        add(shape(GEOMS[0], (4, 192), ci, 0, 128), opt(pro=pro), t)
        add(shape(GEOMS[2], (4, 192), ci, 0, 128), opt(pro=pro), t)
    return rows


def rows_sha256(rows):
    return hashlib.sha256(repr(rows).encode()).hexdigest()


def pack_answers(rows, answers, recorded_from):
    """The fixture document of per-row answer tuples (in the rows' order)."""
    table = list(dict.fromkeys(answers))
    assert len(table) <= 256
    index = {a: i for i, a in enumerate(table)}
    blob = base64.b64encode(zlib.compress(bytes(index[a] for a in answers), 9)).decode()
    return {'recorded_from': recorded_from, 'n_rows': len(rows), 'rows_sha256': rows_sha256(rows),
            'answer_keys': ['launched', 'label', 'emits_gn', 'lds_tables', 'drift'],
            'answers': [list(a) for a in table], 'row_answers_zlib_b64': [blob[i:i + 100] for i in range(0, len(blob), 100)]}


def dump_doc(doc):
    """JSON with one answer and 100 characters of the row bytes per line."""
    lines = [f'"{k}": {json.dumps(doc[k])}' for k in ('recorded_from', 'n_rows', 'rows_sha256', 'answer_keys')]
    for k in ('answers', 'row_answers_zlib_b64'):
        lines.append(f'"{k}": [\n' + ',\n'.join(json.dumps(a, separators=(',', ':')) for a in doc[k]) + '\n]')
    return '{\n' + ',\n'.join(lines) + '\n}\n'


def unpack_answers(doc):
    """(rows, their answer tuples) of a fixture document; the enumeration must be the one it was recorded over."""
    rows = enumerate_rows()
    assert len(rows) == doc['n_rows'] and rows_sha256(rows) == doc['rows_sha256'], 'the enumeration changed'
    idx = zlib.decompress(base64.b64decode(''.join(doc['row_answers_zlib_b64'])))
    assert len(idx) == len(rows)
    return rows, [tuple(doc['answers'][i]) for i in idx]


def out_size(s):
    taps, stride, up, pad0, H, W = s[:6]
    if up:
        return 2 * H, 2 * W
    if pad0 and stride == 2:
        return (H - 2) // 2 + 1, (W - 2) // 2 + 1
    if taps == 9 and stride in (1, 2):
        return (H - 1) // stride + 1, (W - 1) // stride + 1
    return H, W


# stand-in addresses (never read): distinct, 16-byte aligned
_X, _X2, _W, _Y, _BIAS, _ROWVEC, _RES, _PRO, _WS, _WINO = (0x10000000 * (i + 1) for i in range(10))


def ask(dmhip, s, o, toggles):
    """One row through dm_debug_conv_choice, with the row's toggles in the environment for the call."""
    sd, od = dict(zip(SHAPE_KEYS, s)), dict(zip(OPT_KEYS, o))
    Hout, Wout = out_size(s)
    bad = od['bad']
    d = dmhip.ConvDesc()
    d.x, d.x_pitch, d.Cin, d.Hin, d.Win = _X, sd['Cin1'] + (2 if bad == 3 else 0), sd['Cin1'], sd['Hin'], sd['Win']
    d.taps, d.stride, d.upsample = sd['taps'], sd['stride'], sd['upsample']
    if sd['Cin2']:
        d.x2, d.x2_pitch, d.Cin2 = _X2, sd['Cin2'], sd['Cin2']
    d.w = _W + (4 if bad == 5 else 0)
    d.K = (4 if sd['upsample'] == 2 else sd['taps']) * sd['Cin1'] + sd['Cin2'] + (32 if bad == 1 else 0)
    d.y = _Y + (4 if od['misalign_y'] else 0)
    d.Cout, d.B, d.Hout, d.Wout = sd['Cout'], sd['B'], Hout - (1 if bad == 2 else 0), Wout
    d.y_pitch = sd['Cout'] + od['pitch_extra'] - (4 if bad == 6 else 0)
    d.bias = _BIAS
    if od['rowvec']:
        d.rowvec, d.rowvec_pitch = _ROWVEC, sd['Cout']
    if od['res']:
        d.res, d.res_pitch = _RES, sd['Cout']
    d.tile = od['tile']
    if od['pro'] == 1:
        d.pro_scale, d.pro_shift = _PRO, _PRO + 0x100000
    d.pro_nosilu = od['nosilu']
    if od['weights'] and bad != 4:
        d.w_split, d.w_split_kind = _WS, 3 if od['weights'] == 1 else 2
    if od['weights'] >= 3:
        d.w_wino, d.w_wino_fold = _WINO, od['weights'] - 3
    d.ksplit = od['ksplit']
    gin_G = 32 if od['pro'] == 2 else 0
    nchunk = (sd['Hin'] * sd['Win'] + 63) // 64
    saved = {n: os.environ.pop(n, None) for n in TOGGLE_ENV}
    os.environ.update(toggles)
    try:
        return dmhip.conv_choice(d, s2_pad0=sd['s2_pad0'], gn_G=od['gn_G'], gn_emit=od['gn_emit'],
                                 pick_B=od['pick_B'], ksplit_has_part=int(od['ksplit'] > 1 and bad != 7), h16=od['h16'], gin_G=gin_G,
                                 gin_nchunk=nchunk)
    finally:
        for n, v in saved.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


# The kernel a `launched` answer runs, as a pattern of its profile label (rocprofv3's name, spaces removed).
_B = '(true|false)'
_K32 = {
    't128x128': rf'128,128,64,64,{_B},false,{_B}>', 't128x64': rf'128,64,64,32,{_B},false,{_B}>',
    'splitk64x64': rf'64,64,32,32,{_B},true,false>', 'splitk64x128': rf'64,128,32,64,{_B},true,false>',
    'seg64': rf'64,128,32,64,{_B},false,{_B}>', 'rows64': rf'64,128,32,64,{_B},false,false>',
    'wide512': rf'128,128,64,32,{_B},false,{_B},512>', 'bigtab': rf'128,128,64,64,{_B},false,{_B},256,208,8192>',
    's2': rf'64,128,32,32,{_B},false,false,512,392,2048,true>',
    's2seg': rf'64,128,32,32,{_B},false,false,512,392,2048,true>',
    't2d': rf'128,128,64,64,{_B},false,{_B},256,208,2048,false,true>',
}


def label_pattern(launched):
    fam, var = launched.split(':')
    if fam == 'im2col':
        return rf'conv_igemm_kernel<{var.replace("x", ",")},\d+,\d+,[0-3]>'
    if fam == 'patch':
        return rf'conv_patch_kernel<{var.replace("x", ",")},\d+,\d+,[0-2],\d+,{_B},{_B}>'
    if fam == 'patch3':
        if var == 'seg128':
            return rf'conv_patch3_kernel<128,128,64,64,[0-2],392,{_B},false,2>'
        return rf'conv_patch3_kernel<{var.replace("x", ",")},\d+,\d+,[0124],(?!392)\d+,{_B},{_B},[23]>'
    if fam == 'pw3':
        return rf'conv_patch3_kernel<{var.replace("x", ",")},64,\d+,3,128,{_B},false,2>'
    if fam == 'k32':
        return 'conv_k32_kernel<' + _K32[var]
    if fam == 'k32small':
        return rf'conv_k32s_kernel<{_B},{var[1:]}>'
    if fam == 'wino':
        return rf'conv_wino_wide_kernel<[0-2],{_B}>' if var == 'wide' else rf'conv_wino_kernel<{var[1:]},[0-2],{_B}>'
    if fam == 'subwino':
        return rf'conv_subwino_kernel<{var[1:]},0>'
    if fam == 'h16':
        return rf'conv_h16_kernel<{"true" if var == "t2d" else "false"},(32|64)>'
    raise ValueError(launched)


def label_names_launched(label, launched):
    return re.fullmatch(label_pattern(launched), label) is not None
