"""The sub-pixel Winograd form of nearest-2x + 3x3 conv (conv_subwino.hip), restated in float64 on the CPU.

Along x, for low-res pixel j and the tap-row weights g = (g0, g1, g2):
    V0 = x[j-1] - x[j]   V1 = x[j]             V2 = x[j+1] - x[j]      (x = 0 outside the map)
    U0 = g0              U1 = g0 + g1 + g2     U2 = g2
    m_b = sum over (channel, tap row) of V_b U_b,   out[2j] = m0 + m1,   out[2j+1] = m1 + m2
Along y the sum stays direct in the sub-pixel form: output row 2i takes low-res rows i - 1 and i with the weights
w_y0 and w_y1 + w_y2, output row 2i + 1 rows i and i + 1 with w_y0 + w_y1 and w_y2: 12 products per low-res pixel and
(cin, cout) pair where the four 4-tap sub-pixel convs take 16."""
import pytest
import torch
import torch.nn.functional as F


def subwino_u(w):
    """The six U matrices of a 3x3 weight [Cout][Cin][3][3]: U[py][ty][b] of shape [Cout][Cin]."""
    w = w.double()
    rows = [[w[:, :, 0, :], w[:, :, 1, :] + w[:, :, 2, :]],   # py 0: low-res rows i - 1, i
            [w[:, :, 0, :] + w[:, :, 1, :], w[:, :, 2, :]]]   # py 1: low-res rows i, i + 1
    return [[[g[..., 0], g[..., 0] + g[..., 1] + g[..., 2], g[..., 2]] for g in rows[py]] for py in range(2)]


def subwino_v(x):
    """The three V planes of a low-res map [B][Cin][H][W] (zero outside the map)."""
    x = x.double()
    xp = F.pad(x, (1, 1))
    return [xp[..., :-2] - x, x, xp[..., 2:] - x]


def subwino_conv(x, w, bias=None):
    """nearest-2x + 3x3 conv (padding 1) of x [B][Cin][H][W] by the plane formula, in float64."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    U, V = subwino_u(w), subwino_v(x)
    Vp = [F.pad(v, (0, 0, 1, 1)) for v in V]  # one zero row above and below
    out = torch.zeros((B, Cout, 2 * H, 2 * W), dtype=torch.float64)
    for py in range(2):
        m = []
        for b in range(3):
            acc = torch.zeros((B, Cout, H, W), dtype=torch.float64)
            for ty in range(2):
                r = py + ty  # padded row offset: low-res row i - 1 + py + ty
                acc += torch.einsum('bchw,oc->bohw', Vp[b][:, :, r:r + H, :], U[py][ty][b])
            m.append(acc)
        out[:, :, py::2, 0::2] = m[0] + m[1]
        out[:, :, py::2, 1::2] = m[1] + m[2]
    if bias is not None:
        out += bias.double()[None, :, None, None]
    return out


def _ref(x, w, bias=None):
    return F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(),
                    None if bias is None else bias.double(), padding=1)


@pytest.mark.parametrize('B,Cin,Cout,H,W', [(2, 3, 4, 4, 4), (1, 5, 2, 7, 5), (2, 2, 3, 1, 6), (1, 4, 2, 6, 1),
                                            (1, 1, 1, 1, 1), (3, 2, 2, 3, 16), (1, 3, 5, 8, 8)])
def test_plane_formula_matches_upsampled_conv(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(100 + H * 17 + W)
    x = torch.randn((B, Cin, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn((Cout, ), generator=g, dtype=torch.float64)
    assert (subwino_conv(x, w, b) - _ref(x, w, b)).abs().max().item() <= 1e-12


@pytest.mark.parametrize('py,px', [(0, 0), (0, 2), (2, 0), (2, 2), (1, 1), (0, 1), (1, 0), (2, 1), (1, 2)])
def test_single_tap_single_pixel_at_the_edges(py, px):
    """One non-zero tap against one non-zero pixel at every corner, edge and the middle: the zero padding of V (x
    outside the map) and of the rows above / below, and the parity each product lands in."""
    H, W = 3, 4
    w = torch.zeros((1, 1, 3, 3), dtype=torch.float64)
    w[0, 0, py, px] = 1.5
    for iy in range(H):
        for ix in range(W):
            x = torch.zeros((1, 1, H, W), dtype=torch.float64)
            x[0, 0, iy, ix] = 2.0
            assert (subwino_conv(x, w) - _ref(x, w)).abs().max().item() <= 1e-12, (iy, ix)


def test_product_count():
    """2 py x 3 planes x 2 tap rows = 12 matrices of [Cout][Cin] against 16 of the four 4-tap sub-pixel convs."""
    U = subwino_u(torch.zeros((2, 3, 3, 3)))
    assert sum(len(U[py][ty]) for py in range(2) for ty in range(2)) == 12
