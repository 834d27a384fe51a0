"""The tiled plan off the power-of-two grids, on the CPU emulator: the shape matrix S1-S4 of tests/tiled_shapes.py (24x24 with attention
over 144 positions, 16x24, 8x8 at nf 32 with attention over 16 positions, 16x16 at nf 96) against the float64 torch oracle.
tests/test_gpu_tiled_shapes.py runs the same checks on an MI355X."""
import ctypes as C

import pytest

from tests import tiled_shapes as S

DEV = 'cpu'


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4'])
def test_forward_matches_float64_oracle(emu, name, dtype):
    """Classifier-free-guidance score, B = 3 (6 forwards), weights 0 / 0.6 / 1.5, t = 0.15 / 0.5 / 0.85: per sample
    max |s - ref64| <= tol max |ref64|, tol = 2e-5 (fp32) and 3e-2 (bf16 operands), the project's stated tolerances.
    Measured here (emulator), per sample:      fp32                        bf16
      S1  24x24 attn L=144                     6.0e-6 2.4e-6 4.1e-6         1.22e-2 1.13e-2 1.06e-2
      S2  16x24                                6.2e-6 2.7e-6 3.6e-6         1.37e-2 1.19e-2 9.2e-3
      S3  8x8 nf 32 attn L=16                  3.8e-6 1.7e-6 4.0e-6         8.8e-3 1.02e-2 1.00e-2
      S4  16x16 nf 96                          4.3e-6 3.2e-6 4.7e-6         1.20e-2 1.47e-2 1.34e-2
    S1 and S3 in bf16 are the regression tests of bgemm_nt_bf16_kernel's last K step (P V contracts K = L = 144 / 16): before it was
    predicated, S1 bf16 measured 1.25e-1 / 1.25e-1 / 9.6e-2 (and S3 4.9e-1 / 4.8e-1 / 9.6e-1) with no error raised."""
    S.check_forward(name, dtype, DEV)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['S1', 'S4'])
def test_wide_workgroups(emu, name, dtype, monkeypatch):
    """RDMI_TILED_MIN_WGS=1: NCT = 2 / 4 column tiles per wave and the vector epilogue over masked row tails (S1) and over a padded
    width of one and a half workgroups (S4).  fp32 within 2e-5 of the oracle; bf16 bit-identical to the narrow run, as
    test_cifar_bf16_vector_epilogue_is_bit_identical asserts for CIFAR (and so within 3e-2).
    Measured here (emulator): S1 fp32 6.0e-6 / 2.4e-6 / 4.1e-6 (the narrow run's figures), S4 fp32 4.3e-6 / 3.2e-6 / 4.7e-6."""
    narrow = S.cf_score(name, dtype, DEV)
    monkeypatch.setenv('RDMI_TILED_MIN_WGS', '1')
    wide = S.check_forward(name, dtype, DEV, wide=True)
    if dtype == 'bf16':
        assert bool((wide == narrow).all()), float((wide - narrow).abs().max())


@pytest.mark.parametrize('name', ['S1', 'S2'])
def test_short_tile_statistics_with_large_group_means(emu, name, monkeypatch):
    """Every conv bias + 40 (test_tiled_plan_groupnorm_statistics_with_large_group_means) on the grids whose last tile is short (12x12:
    tiles of 5, 5 and 2 rows; 8x12: 5 and 3 rows): a wrong pixel count of the last tile in the Chan merge shifts the group mean by a
    fraction of 40.  fp32, against the float64 oracle and against the two-pass statistics (RDMI_TILED_STATS_PASS=1), 1e-4 max |ref|.
    Measured here (emulator): S1 2.1e-6 / 2.4e-6 of max |ref| against the oracle, 2.2e-6 / 2.1e-6 against the two-pass run, S2 2.0e-6 / 1.9e-6 and 2.5e-6 / 1.9e-6."""
    S.check_shifted_statistics(name, DEV, monkeypatch)


def test_taps_localise_attention_and_12x12_block(emu):
    """S1, fp32: the attention blocks' outputs (L = 144) and the last 12x12 residual block against the oracle's intermediates,
    1e-4 max(1, max |tap|).  Measured here (emulator): max |tap - ref64| 1.1e-5 (down_attn.1), 1.8e-5 (up_attn.3), 1.8e-5 (up_blocks.3) on max |tap| 2.5-2.8."""
    S.check_taps('S1', DEV, ['down_attn.1', 'up_attn.3', 'up_blocks.3'])


def test_backward_matches_float64_autograd(emu):
    """S2, fp32 tiled training plan, B = 2, dropout off: every parameter gradient ||g - g64|| <= 1e-4 ||g64|| (the key-bias exception of
    tests/test_emu_tiled_train.py does not arise: no attention), grad_x of the full and of the VJP-only call whole / per channel /
    border frame at 1e-4.  S1 (attention over 144 positions, three-tile images) runs on the GPU only: the emulator needs four minutes for
    it (run once by hand here: worst parameter gradient 7.1e-6, grad_x 3.2e-6 in both modes).
    Measured here (emulator): worst parameter gradient 4.9e-6, grad_x 3.4e-6 in both modes."""
    S.check_backward('S2', DEV)


def test_groupnorm_group_divisibility_is_checked(emu):
    """nf 48 with ch_mult (1, 2, 2): the 144-channel concatenation would get min(144 / 4, 32) = 32 groups, which torch.nn.GroupNorm refuses
    (so the Python module never reaches the library): rdmi_create must refuse it too, for every plan, naming the tensor."""
    for H, W, channels in ((16, 16, 3), (9, 9, 1)):             # tiled plan / the workgroup-resident and layer plans
        a = emu.Arch()
        a.nf, a.n_levels, a.num_res_blocks, a.attn_levels, a.channels = 48, 3, 1, 0, channels
        a.ch_mult[0], a.ch_mult[1], a.ch_mult[2] = 1, 2, 2
        a.num_classes, a.conditional, a.scale_by_sigma = 1, 1, 1
        h = C.c_void_p()
        rc = emu.lib().rdmi_create(C.byref(a), 2, H, W, C.byref(h))
        msg = emu.lib().rdmi_last_error().decode()
        assert rc != 0 and not h.value, msg
        assert 'up_blocks.4.GroupNorm_0' in msg and '144' in msg and 'divisible' in msg, msg
