"""The tiled plan off the power-of-two grids, on an MI355X: the checks of tests/test_emu_tiled_shapes.py (shape matrix S1-S4 of
tests/tiled_shapes.py against the float64 torch oracle) on the device, plus the backward of S1."""
import pytest

from tests import tiled_shapes as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _device_library():
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4'])
def test_forward_matches_float64_oracle(name, dtype):
    """As tests/test_emu_tiled_shapes.py::test_forward_matches_float64_oracle: per sample max |s - ref64| <= tol max |ref64|, tol = 2e-5
    (fp32) and 3e-2 (bf16).  Not yet measured on an MI355X (the figures are printed by the check: run with -s); the emulator, which
    runs the same kernels, measured 1.7e-6 .. 6.2e-6 (fp32) and 8.8e-3 .. 1.47e-2 (bf16): see the emulator test's table."""
    S.check_forward(name, dtype, DEV)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['S1', 'S4'])
def test_wide_workgroups(name, dtype, monkeypatch):
    """RDMI_TILED_MIN_WGS=1 (NCT = 2 / 4 and the vector epilogue over masked tails): fp32 within 2e-5 of the oracle, bf16 bit-identical to
    the narrow run.  Not yet measured on an MI355X; emulator: 6.0e-6 (S1 fp32), 4.7e-6 (S4 fp32) at the worst sample."""
    narrow = S.cf_score(name, dtype, DEV)
    monkeypatch.setenv('RDMI_TILED_MIN_WGS', '1')
    wide = S.check_forward(name, dtype, DEV, wide=True)
    if dtype == 'bf16':
        assert bool((wide == narrow).all()), float((wide - narrow).abs().max())


@pytest.mark.parametrize('name', ['S1', 'S2'])
def test_short_tile_statistics_with_large_group_means(name, monkeypatch):
    """Every conv bias + 40 on the grids whose last tile is short: fp32 against the float64 oracle and the two-pass statistics,
    1e-4 max |ref|.  Not yet measured on an MI355X; emulator: 2.4e-6 (S1), 2.0e-6 (S2) against the oracle."""
    S.check_shifted_statistics(name, DEV, monkeypatch)


def test_taps_localise_attention_and_12x12_block():
    """S1, fp32: attention block outputs (L = 144) and the last 12x12 residual block against the oracle's intermediates,
    1e-4 max(1, max |tap|).  Not yet measured on an MI355X; emulator: 1.1e-5 .. 1.8e-5 on max |tap| 2.5 .. 2.8."""
    S.check_taps('S1', DEV, ['down_attn.1', 'up_attn.3', 'up_blocks.3'])


@pytest.mark.parametrize('name', ['S1', 'S2'])
def test_backward_matches_float64_autograd(name):
    """fp32 tiled training plan, B = 2, dropout off: every parameter gradient ||g - g64|| <= 1e-4 ||g64|| (the analytically zero key
    bias NIN_1.b against the floor of tests/test_emu_tiled_train.py), grad_x of the full and of the VJP-only call whole / per channel /
    border frame at 1e-4.  Not yet measured on an MI355X; emulator: worst parameter gradient 7.1e-6 (S1), 4.9e-6 (S2),
    grad_x 3.2e-6 / 3.4e-6."""
    S.check_backward(name, DEV)
