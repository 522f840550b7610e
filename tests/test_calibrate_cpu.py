"""The shapes tests/test_calibrate_gpu.py calibrates at are well conditioned: at each of them, for each variant, the float32 CPU
oracle's calibration lies within ONE bound (1e-4 * max(1, |ref64|), oracle/report.py) of the float64 one, and no float64 variance is
below 5e-3.  Below these shapes neither holds (fewer than about 9 rows at the coarsest grid: a variance near 0, and the folded
1 / sqrt(var + 1e-5) amplifies rounding by up to 316 per layer) and a device test there would measure the conditioning of the
network, not byolo_calibrate_bn.  Runs without a GPU; the oracle pairs are the ones the GPU test compares the device with."""
import pytest

from _calibrate_ref import VARIANTS, SHAPES, MIN_VARIANCE, MEAN, VAR, oracle_pair, bn_scopes


@pytest.mark.parametrize("H,W,B", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_calibration_shapes_are_well_conditioned(variant, H, W, B):
    o = oracle_pair(variant, H, W, B)
    print("%s %dx%d B=%d: F means %.3f (%s), F variances %.3f (%s), smallest variance %.4g, %d BN layers"
          % (variant, H, W, B, o["F"][MEAN], o["floor"][MEAN]["worst_layer"], o["F"][VAR], o["floor"][VAR]["worst_layer"], o["min_var"],
             len(o["scopes"])))
    assert o["floor"][MEAN]["layers"] == o["floor"][VAR]["layers"] == len(bn_scopes(variant)) == 72
    assert o["F"][MEAN] < 1 and o["F"][VAR] < 1, o["F"]
    assert o["min_var"] >= MIN_VARIANCE, o["min_var"]
