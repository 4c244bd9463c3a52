"""Host side of the guided samplers (diffusions/guidance/): RePaint resample sequences, the low-pass filter's
axis tables, error cases and the C ABI declarations. No GPU needed.

Fixtures: tests/golden/guidance.npz, generated from the reference modules (tests/golden/make_golden_guidance.py).
"""
import re

import numpy as np
import pytest
import torch

import dmhip
from diffusions import ILVR, BaseGuidance, MaskGuidance
from diffusions.guidance import lowpass

NEW_SYMBOLS = ['dm_guided_step', 'dm_lowpass_create', 'dm_lowpass_apply', 'dm_lowpass_scratch_bytes',
               'dm_lowpass_destroy']


def test_resample_sequences_equal_the_reference(golden):
    arrays, meta = golden('guidance')
    assert [4, 2, 2] in meta['seq_cases'] and [20, 2, 5] in meta['seq_cases']
    assert any(r == 1 for _, r, _ in meta['seq_cases'])
    for steps, r, j in meta['seq_cases']:
        d = MaskGuidance(respace_type='uniform', respace_steps=steps)
        seq = d.get_resample_seq(r, j)
        assert seq == arrays[f'seq_{steps}_{r}_{j}'].tolist(), (steps, r, j)
    # respace_steps 4, r = 2, j = 2: 8 steps, two of them forward q-steps
    seq = arrays['seq_4_2_2'].tolist()
    assert len(seq) == 8 and sum(a < b for a, b in zip(seq, seq[1:])) == 2


def test_axis_tables_match_the_reference_matrices(golden):
    """The densified host tables against the reference resize of an identity; rtol / atol: the project's bound
    for host-dependent torch rounding (tests/test_gpu_samplers.py)."""
    arrays, meta = golden('guidance')
    assert [256, 8, 'cubic'] in meta['mats']
    for size, n, method in meta['mats']:
        dh, dw, uh, uw = lowpass.axis_tables(size, size, n, method)
        for tab in (dh, dw):
            got = lowpass.densify(tab, size, torch.float32).numpy()
            assert np.allclose(got, arrays[f'mat_down_{size}_{n}_{method}'], rtol=1e-5, atol=2e-5), (size, n, method)
        for tab in (uh, uw):
            got = lowpass.densify(tab, size // n, torch.float32).numpy()
            assert np.allclose(got, arrays[f'mat_up_{size}_{n}_{method}'], rtol=1e-5, atol=2e-5), (size, n, method)
        # every row normalised (rows whose field of view leaves the axis lose the padded taps)
        w = dh[0]
        assert np.allclose(w.sum(1).numpy(), 1.0, atol=1e-5)


def test_tables_reproduce_the_reference_low_pass_filter(golden):
    """The four tables chained in float64 give the reference's low_pass_filter output (its fp32 rounding apart)."""
    arrays, meta = golden('guidance')
    for h, w, n, method in meta['lp_cases']:
        dh, dw, uh, uw = lowpass.axis_tables(h, w, n, method)
        x = torch.from_numpy(arrays[f'lp_{h}_{w}_{n}_{method}_x']).double()
        mh = lowpass.densify(uh, h // n) @ lowpass.densify(dh, h)
        mw = lowpass.densify(uw, w // n) @ lowpass.densify(dw, w)
        y = mh @ x @ mw.T
        err = (y - torch.from_numpy(arrays[f'lp_{h}_{w}_{n}_{method}_y']).double()).abs().max().item()
        assert err <= 1e-5, (h, w, n, method, err)


def test_error_cases():
    with pytest.raises(ValueError):
        lowpass.axis_tables(32, 32, 5, 'cubic')
    with pytest.raises(ValueError):
        lowpass.axis_tables(32, 24, 16, 'cubic')
    with pytest.raises(ValueError):
        lowpass.axis_tables(32, 32, 4, 'nearest')
    with pytest.raises(ValueError):
        ILVR(downsample_factor=5).low_pass_filter(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        ILVR(interp_method='nearest')
    z = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match='set_mask_and_image'):
        MaskGuidance().cond_fn_sample(t=10, t_prev=9, sample=z)
    with pytest.raises(RuntimeError, match='set_mask_and_image'):
        MaskGuidance(masked_image=z).cond_fn_sample(t=10, t_prev=9, sample=z)
    with pytest.raises(RuntimeError, match='set_ref_images'):
        ILVR().cond_fn_sample(t=10, t_prev=9, sample=z)
    with pytest.raises(ValueError):
        MaskGuidance(var_type='nope')


def test_fused_step_only_for_the_classes_own_guidance():
    """A subclass that overrides any hook goes through the generic apply_guidance path."""
    class Sub(MaskGuidance):
        def cond_fn_x0(self, **kw):
            return None

    class Same(ILVR):
        pass
    assert MaskGuidance()._fused() and ILVR()._fused() and Same()._fused()
    assert not Sub()._fused() and not BaseGuidance()._fused()


def test_header_declares_the_guidance_abi():
    names = dmhip.exported_symbols()
    for n in NEW_SYMBOLS:
        assert n in names, n
    L = dmhip.load()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    hdr = open(dmhip._lib._HEADER).read()
    assert int(re.search(r'#define DM_ABI_VERSION (\d+)', hdr).group(1)) == 2 == L.dm_abi_version()
    assert 'typedef struct dm_guide_desc' in hdr and 'mode 3' in hdr
    # the ctypes mirror has the header's fields in order
    body = re.search(r'typedef struct dm_guide_desc \{(.*?)\} dm_guide_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [re.split(r'[\s\*]+', d.strip())[-1] for stmt in body.split(';') for d in stmt.split(',') if d.strip()]
    assert fields == [f[0] for f in dmhip.GuideDesc._fields_], fields
