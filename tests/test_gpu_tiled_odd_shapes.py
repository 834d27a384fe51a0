"""The tiled plan on odd level grids and with attention over L % 16 != 0 positions, on an MI355X: the shape matrix O1-O4 of
tests/tiled_odd_shapes.py (10x10x1 with attention over 100 positions, 11x11x1 with attention over 25, 9x9x3 with attention over 81,
10x14x3) against the float64 torch oracle: forward in fp32 and bf16, wide workgroups, shifted statistics, taps, the fp32 backward with
input gradients, and O1 through the fused sampler loop.  Before the nearest resize and the padded attention rows were built,
rdmi_create refused every one of these shapes."""
import pytest

from tests import tiled_odd_shapes as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _device_library():
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['O1', 'O2', 'O3', 'O4'])
def test_forward_matches_float64_oracle(name, dtype):
    """Classifier-free-guidance score, B = 3: per sample max |s - ref64| <= tol max |ref64|, tol = 2e-5 (fp32) and 3e-2 (bf16); path_info
    reports the tiled plan and 1 / 2 / 1 / 1 resize launches.  Measured on an MI355X, worst sample (the check prints all; run with -s):
      O1 fp32 1.19e-5, bf16 2.79e-2 (the samples: 1.66e-2 / 2.79e-2 / 1.39e-2; the emulator gives 2.75e-2 for the same sample)
      O2 fp32 1.20e-5, bf16 1.79e-2        O3 fp32 6.9e-6, bf16 1.57e-2        O4 fp32 5.8e-6, bf16 1.16e-2
    O1's bf16 figure is that of full-resolution attention at C = 32 in this small network, not of the padded rows: the same model at
    12x12x1 (L = 144, no pad, no resize) measures 2.9e-2 on the emulator, and 10x10x1 without attention 1.6e-2."""
    S.check_forward(name, dtype, DEV)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_wide_workgroups(dtype, monkeypatch):
    """O2 with RDMI_TILED_MIN_WGS=1: fp32 within 2e-5 of the oracle, bf16 bit-identical to the narrow run."""
    narrow = S.cf_score('O2', dtype, DEV)
    monkeypatch.setenv('RDMI_TILED_MIN_WGS', '1')
    wide = S.check_forward('O2', dtype, DEV, wide=True)
    if dtype == 'bf16':
        assert bool((wide == narrow).all()), float((wide - narrow).abs().max())


def test_statistics_of_resized_tensors_with_large_group_means(monkeypatch):
    """O2, every conv bias + 40: fp32 against the float64 oracle and the two-pass statistics, 1e-4 max |ref| (the GroupNorm over a
    resized tensor must not use the producer's channel records)."""
    S.check_shifted_statistics('O2', DEV, monkeypatch)


@pytest.mark.parametrize('name,taps', [('O1', ['down_attn.0', 'up_attn.5', 'up_blocks.2']), ('O2', ['down_attn.1', 'up_attn.3', 'up_blocks.2', 'up_blocks.4'])])
def test_taps_localise_attention_and_first_resized_block(name, taps):
    """fp32: attention block outputs (L = 100 / 25) and the up blocks that read a resized h against the oracle's intermediates,
    1e-4 max(1, max |tap|)."""
    S.check_taps(name, DEV, taps)


@pytest.mark.parametrize('name', ['O1', 'O2', 'O3'])
def test_backward_matches_float64_autograd(name):
    """fp32 tiled training plan, B = 2, dropout off: every parameter gradient ||g - g64|| <= 1e-4 ||g64|| (NIN_1.b against the floor of
    tests/test_emu_tiled_train.py), grad_x of the full and of the VJP-only call whole / per channel / border frame at 1e-4; a second round
    of the three backward calls is bit-identical to the first."""
    S.check_backward(name, DEV)


@pytest.mark.parametrize('corrector', ['none', 'langevin'])
def test_fused_sampler_loop(corrector):
    """O1 through get_pc_sampler(fused=True), N = 4 scales, injected noise, teacher-forced: the trace after each of the 3 updates against
    OT.pc_update in float64 fed the same draws, at the tolerance of test_gpu_cifar.py's tiled updates."""
    S.check_sampler('O1', DEV, corrector)
