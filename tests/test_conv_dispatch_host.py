"""The conv dispatch against its recorded fixture (tests/golden/conv_dispatch.json, tests/conv_dispatch_ref.py).

Every row of the fixture -- a conv descriptor, the options the plans set beside it and a toggle setting -- is asked
again of the built library through dm_debug_conv_choice (host only: no GPU, stand-in addresses), and the kernel it
would launch, whether it can emit GroupNorm statistics, whether it stages its tables in LDS and whether it is refused
must equal the record. The label must equal the record too, except on rows the generator marked as drift (the
recorded label did not name the recorded kernel): there it must name the launched kernel.

The fixture was recorded once, from the commit in its "recorded_from" field, before conv_choose replaced the three
hand-kept copies of the dispatch; it is not regenerated with the code.
"""
import collections
import json
import os

import pytest

from tests import conv_dispatch_ref as ref
from tests.conftest import GOLDEN

# "family:variant" answers of conv_choose (csrc/dm_kernels.h ConvFamily and the per-family variant enums)
ALL_LAUNCHED = (
    ['im2col:128x128', 'im2col:128x64', 'im2col:64x64', 'patch:128x128', 'patch:128x64', 'patch:64x64'] +
    ['patch3:128x128', 'patch3:128x64', 'patch3:64x64', 'patch3:256x256', 'patch3:512x128', 'patch3:seg128'] +
    ['pw3:128x128', 'pw3:128x64'] +
    ['k32:' + v for v in ('t128x128', 't128x64', 'splitk64x64', 'splitk64x128', 'seg64', 'wide512', 'bigtab', 's2',
                          't2d', 'rows64', 's2seg')] +
    ['k32small:w8', 'k32small:w4'] + ['wino:w32', 'wino:w16', 'wino:w8', 'wino:w4', 'wino:wide'] +
    ['subwino:w16', 'subwino:w8', 'subwino:w4'] + ['h16:rows', 'h16:t2d'])
# reachable by a forced tile only
FORCED_ONLY = {
    'patch3:256x256': 'tile 7: conv_patch_pick keeps the one-wave-per-SIMD split tiles behind tiles 7 / 8',
    'patch3:512x128': 'tile 8: as tile 7',
    # the automatic K32 choice starts from a 128-row halo-patch pick, which needs >= 512 blocks of 128 x 64, and takes
    # 128 x 128 tiles from 256 blocks of those on: never fewer than 256 when there are 512 of half the width
    'k32:t128x64': 'tile 11: the automatic choice always finds >= 256 blocks of 128 x 128 where it looks',
    # the gate of the 64 x 64 split-K tiles is the gate of the 64 x 128 ones, which the automatic choice tries first
    'k32:splitk64x64': 'tile 12: wherever it fits, so do the 64 x 128 split-K tiles',
}


@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(GOLDEN, 'conv_dispatch.json')) as f:
        doc = json.load(f)
    return doc


def _rows(doc):
    rows, answers = ref.unpack_answers(doc)
    for (s, o, t), (launched, label, emits, lds, drift) in zip(rows, answers):
        yield s, dict(zip(ref.OPT_KEYS, o)), t, launched, label, emits, lds, drift


def test_fixture_is_not_vacuous(fixture):
    rows = list(_rows(fixture))
    n = len(rows)
    auto, taken, not_taken = set(), collections.Counter(), collections.Counter()
    for s, o, t, launched, label, emits, lds, drift in rows:
        if o['tile'] == 0:
            auto.add(launched)
        elif 1 <= o['tile'] <= 23 and not o['h16']:  # (the conv-half mark reads tile as its own form number)
            (taken if o['tile'] in _forms_of(launched) else not_taken)[o['tile']] += 1
    for name in ALL_LAUNCHED:
        assert name in auto or name in FORCED_ONLY, f'{name}: no tile-0 row launches it'
    for name in FORCED_ONLY:
        assert any(r[3] == name for r in rows), f'{name}: no row launches it'
    for tile in range(1, 24):
        assert taken[tile] > 0, f'tile {tile}: no row takes it'
        assert not_taken[tile] > 0, f'tile {tile}: no row refuses it or falls back'
    assert sum(1 for r in rows if r[3] == 'refused') >= 0.05 * n
    # the Winograd-to-direct fallback: an automatic conv with Winograd weights that runs the Winograd kernel without
    # statistics, and a direct kernel when asked for statistics the Winograd epilogue cannot emit
    wino = {(s, t) for s, o, t, launched, *_ in rows
            if o == dict(zip(ref.OPT_KEYS, ref.opt(weights=3))) and launched.startswith('wino:')}
    fell_back = [r for r in rows if r[1]['weights'] == 3 and r[1]['tile'] == 0 and r[1]['gn_emit'] and not r[1]['pro']
                 and not r[1]['h16'] and (r[0], r[2]) in wino and r[3] != 'refused' and not r[3].startswith('wino:')]
    assert fell_back, 'no row exercises the Winograd-to-direct fallback'
    assert all(r[5] == 1 for r in fell_back)  # the direct kernel it fell back to does emit them


def _forms_of(launched):
    """The forced tile numbers (dm_conv_desc.tile) that name this kernel form (the tile table)."""
    table = {'im2col:128x128': (1, ), 'im2col:128x64': (2, ), 'im2col:64x64': (3, ),
             'patch:128x128': (4, ), 'patch:128x64': (5, ), 'patch:64x64': (6, ),
             'patch3:128x128': (4, ), 'patch3:128x64': (5, ), 'patch3:64x64': (6, ), 'patch3:256x256': (7, ),
             'patch3:512x128': (8, ), 'patch3:seg128': (9, ), 'k32:t128x128': (10, ), 'k32:t128x64': (11, ),
             'k32:splitk64x64': (12, ), 'k32:splitk64x128': (13, ), 'k32:seg64': (14, ), 'k32small:w8': (15, ),
             'k32:wide512': (16, ), 'k32:bigtab': (17, ), 'k32:s2': (18, ), 'k32:t2d': (19, ), 'k32:rows64': (20, ),
             'wino:w32': (21, ), 'wino:w16': (21, ), 'wino:w8': (21, ), 'wino:w4': (21, ), 'wino:wide': (21, ),
             'k32:s2seg': (22, ), 'subwino:w16': (23, ), 'subwino:w8': (23, ), 'subwino:w4': (23, )}
    return table.get(launched, ())


def test_dispatch_equals_the_record(fixture):
    from dmhip import _lib
    _lib.load()
    bad, drift_rows = [], 0
    for s, o, t, launched, label, emits, lds, drift in _rows(fixture):
        got = ref.ask(_lib, s, tuple(o[k] for k in ref.OPT_KEYS), ref.TOGGLES[t])
        want = {'launched': launched, 'emits_gn': emits, 'lds_tables': lds}
        miss = {k: (got[k], v) for k, v in want.items() if got[k] != v}
        if drift:
            drift_rows += 1
            if not ref.label_names_launched(got['label'], got['launched']):
                miss['label'] = (got['label'], 'a label of ' + got['launched'])
        elif got['label'] != label:
            miss['label'] = (got['label'], label)
        if miss:
            bad.append((s, o, ref.TOGGLES[t], miss))
    print(f'{drift_rows} drift rows (recorded label did not name the recorded kernel)')
    assert not bad, f'{len(bad)} rows differ from the record, the first: {bad[:5]}'


def test_labels_name_the_launched_kernel(fixture):
    """Every label in the record that is not marked as drift names the kernel recorded as launched."""
    for s, o, t, launched, label, emits, lds, drift in _rows(fixture):
        if launched != 'refused' and not drift:
            assert ref.label_names_launched(label, launched), (s, o, launched, label)
