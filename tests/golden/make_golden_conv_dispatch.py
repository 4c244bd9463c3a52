"""Golden fixture of the conv dispatch: what every descriptor of tests/conv_dispatch_ref.py's enumeration runs.

Runs on the CPU with the built library (dm_debug_conv_choice makes no HIP call and reads no tensor):
    python tests/golden/make_golden_conv_dispatch.py
Writes tests/golden/conv_dispatch.json (conv_dispatch_ref.pack_answers): per descriptor the answer [launched, label,
emits_gn, lds_tables, drift]. drift = 1 marks a row whose recorded label does not name the kernel recorded as
launched (the label function and the dispatch disagreed in the build the fixture was recorded from);
tests/test_conv_dispatch_host.py holds such a row's label to the launched kernel instead of to the record. Prints the
histogram of the answers and the drift rows by kind.

The fixture records the dispatch of the commit named in its "recorded_from" field and is not regenerated when the
dispatch code is reorganised: it is what a reorganisation is checked against.
"""
import collections
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'diffusion-models-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dmhip  # noqa: E402
from dmhip import _lib  # noqa: E402
from tests import conv_dispatch_ref as ref  # noqa: E402


def main():
    _lib.load()
    rows = ref.enumerate_rows()
    out, hist, drift_kinds = [], collections.Counter(), collections.Counter()
    for s, o, t in rows:
        r = ref.ask(_lib, s, o, ref.TOGGLES[t])
        refused = r['launched'] == 'refused'
        drift = 0 if refused or ref.label_names_launched(r['label'], r['launched']) else 1
        if drift:
            drift_kinds[(r['launched'], r['label'])] += 1
        hist[r['launched']] += 1
        out.append((r['launched'], r['label'], r['emits_gn'], r['lds_tables'], drift))
    head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    doc = ref.pack_answers(rows, out, head)
    path = os.path.join(HERE, 'conv_dispatch.json')
    with open(path, 'w') as f:
        f.write(ref.dump_doc(doc))
    n = len(out)
    print(f'{n} rows, {os.path.getsize(path)} bytes, recorded from {head}')
    for k, v in sorted(hist.items()):
        print(f'  {k:22s} {v:6d}  {100.0 * v / n:5.1f} %')
    print(f'drift rows: {sum(drift_kinds.values())}')
    for (launched, label), v in sorted(drift_kinds.items()):
        print(f'  launched {launched}, labelled {label}: {v}')


if __name__ == '__main__':
    main()
