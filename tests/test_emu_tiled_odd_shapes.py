"""The tiled plan on odd level grids and with attention over L % 16 != 0 positions, on the CPU emulator: shapes O1 (10x10x1, attention
over 100 positions) and O2 (11x11x1, attention over 25 positions at the 5x5 level) of tests/tiled_odd_shapes.py against the float64 torch
oracle.  tests/test_gpu_tiled_odd_shapes.py runs these checks and the rest of the matrix (O3, O4, the sampler loop) on an MI355X.
Before the nearest resize and the padded attention rows were built, rdmi_create refused every one of these shapes ("skip grid 5x5 != 4x4",
"tiled attention needs ... H*W % 16 == 0")."""
import ctypes as C

import pytest

from tests import tiled_odd_shapes as S

DEV = 'cpu'


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['O1', 'O2'])
def test_forward_matches_float64_oracle(emu, name, dtype):
    """Classifier-free-guidance score, B = 3 (6 forwards), per sample max |s - ref64| <= tol max |ref64|, tol = 2e-5 (fp32) / 3e-2 (bf16),
    and path_info reports the tiled plan with 1 (O1) / 2 (O2) resize launches.
    Measured here (emulator), per sample:      fp32                        bf16
      O1  10x10x1 attn L=100                   7.3e-6 4.0e-6 4.4e-6         1.56e-2 2.75e-2 1.14e-2
      O2  11x11x1 attn L=25                    5.9e-6 2.1e-6 3.5e-6         1.28e-2 1.83e-2 1.40e-2"""
    S.check_forward(name, dtype, DEV)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_wide_workgroups(emu, dtype, monkeypatch):
    """O2 with RDMI_TILED_MIN_WGS=1 (NCT = 2 / 4 column tiles per wave over 25- and 55-pixel tiles): fp32 within 2e-5 of the oracle, bf16
    bit-identical to the narrow run."""
    narrow = S.cf_score('O2', dtype, DEV)
    monkeypatch.setenv('RDMI_TILED_MIN_WGS', '1')
    wide = S.check_forward('O2', dtype, DEV, wide=True)
    if dtype == 'bf16':
        assert bool((wide == narrow).all()), float((wide - narrow).abs().max())


def test_statistics_of_resized_tensors_with_large_group_means(emu, monkeypatch):
    """O2, every conv bias + 40: the GroupNorm over concat(resized h, skip) must not use the producer's channel records (sums over the
    4x4 / 10x10 source grid, while the resized tensor repeats a row and a column); a wrong record shifts the group mean by a fraction
    of 40.  fp32 against the float64 oracle and against the two-pass statistics (RDMI_TILED_STATS_PASS=1), 1e-4 max |ref|."""
    S.check_shifted_statistics('O2', DEV, monkeypatch)


@pytest.mark.parametrize('name,taps', [('O1', ['down_attn.0', 'up_attn.5', 'up_blocks.2']), ('O2', ['down_attn.1', 'up_attn.3', 'up_blocks.2', 'up_blocks.4'])])
def test_taps_localise_attention_and_first_resized_block(emu, name, taps):
    """fp32: the attention blocks' outputs (padded score rows: L = 100 / 25) and up_blocks.2, the first up block that reads a resized h
    (4x4 -> 5x5), against the oracle's intermediates at 1e-4 max(1, max |tap|)."""
    S.check_taps(name, DEV, taps)


def test_backward_matches_float64_autograd(emu):
    """O2, fp32 tiled training plan, B = 2, dropout off: every parameter gradient ||g - g64|| <= 1e-4 ||g64|| (NIN_1.b against the floor
    of tests/test_emu_tiled_train.py), grad_x of the full and of the VJP-only call whole / per channel / border frame at 1e-4, and a
    second round of the three backward calls bit-identical to the first (the resize adjoint has one writer per source element)."""
    S.check_backward('O2', DEV)


def _arch(emu, attn_levels, nf=32):
    a = emu.Arch()
    a.nf, a.n_levels, a.num_res_blocks, a.attn_levels, a.channels = nf, 3, 1, attn_levels, 1
    a.ch_mult[0], a.ch_mult[1], a.ch_mult[2] = 1, 2, 2
    a.num_classes, a.conditional, a.scale_by_sigma = 1, 1, 1
    return a


def test_mid_attention_and_narrow_attention_are_still_refused(emu):
    """Attention at the bottleneck resolution (mid_attn) and an attention block whose C is no multiple of 32 stay refused, by name."""
    for a, needle in ((_arch(emu, 0b100), 'mid_attn'), (_arch(emu, 0b001, nf=16), 'tiled attention needs C % 32 == 0')):
        h = C.c_void_p()
        rc = emu.lib().rdmi_create(C.byref(a), 2, 10, 10, C.byref(h))
        msg = emu.lib().rdmi_last_error().decode()
        assert rc != 0 and not h.value, msg
        assert needle in msg, msg
