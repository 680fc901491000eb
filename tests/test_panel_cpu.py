"""Which convs are offered to the row-panel kernel (graph/fused.py
panel_eligible, panel_key; kernels/panel.hip conv1x1_panel_forms): ResNet-50's
three identity-block expand convs are, under a key kind of their own; a reduce
conv, a 3x3 and a stride-2 1x1 are not.  Host code only: no GPU."""
import pytest

from rust_tensorflow_serving2_amd.graph import fused

try:
    from rust_tensorflow_serving2_amd.ops import hip
    H = hip()
except Exception as e:      # the extension is not built / not loadable here
    pytest.skip(f"_hip not importable: {e}", allow_module_level=True)

NOPAD = (0, 0, 0, 0)
# (input NHWC at batch 32, cout) of the stage-2, -3 and -4 expand convs
EXPAND = [((32, 28, 28, 128), 512), ((32, 14, 14, 256), 1024), ((32, 7, 7, 512), 2048)]


@pytest.mark.parametrize("shape,cout", EXPAND)
def test_expand_convs_are_eligible(shape, cout):
    cin = shape[3]
    for act in ("relu", "none"):
        assert fused.panel_eligible(1, 1, 1, 1, NOPAD, cin, cout, act)
    for has_res in (True, False):
        assert fused.panel_key(shape, cout, has_res, "relu") == ("panel", shape, cout, has_res, "relu")
    m = shape[0] * shape[1] * shape[2]
    forms = H.conv1x1_panel_forms(m, cout, cin)
    assert 1 <= len(forms) <= 6 and len(set(forms)) == len(forms)
    for bm, ns in forms:
        assert H.conv1x1_panel_supported(m, cout, cin, bm, ns)
        assert -(-m // bm) * ns >= 128           # each of these shapes has forms with >= 128 workgroups


def test_the_forms_the_issue_names_are_offered():
    assert (64, 1) in H.conv1x1_panel_forms(32 * 28 * 28, 512, 128)
    assert (128, 4) in H.conv1x1_panel_forms(32 * 14 * 14, 1024, 256)
    assert (64, 8) in H.conv1x1_panel_forms(32 * 7 * 7, 2048, 512)
    # no form reaches 128 workgroups: every supported form is offered instead of none
    assert H.conv1x1_panel_forms(128, 512, 128)
    assert H.conv1x1_panel_forms(128, 512, 64) == []         # a depth the kernel is not built for


def test_other_convs_are_not():
    assert not fused.panel_eligible(1, 1, 1, 1, NOPAD, 1024, 256, "relu")        # a reduce conv
    assert not fused.panel_eligible(3, 3, 1, 1, (1, 1, 1, 1), 128, 512, "relu")  # a 3x3
    assert not fused.panel_eligible(1, 1, 2, 2, NOPAD, 256, 1024, "none")        # a stride-2 projection
    assert not fused.panel_eligible(1, 1, 1, 1, NOPAD, 128, 512, "relu6")
    assert not fused.panel_eligible(1, 1, 1, 1, NOPAD, 128, 512, "relu", post=("s", "t", "relu"))
    assert not fused.panel_eligible(1, 1, 1, 1, NOPAD, 64, 256, "relu")          # stage 1: K = 64
    assert not fused.panel_eligible(1, 1, 1, 1, NOPAD, 128, 192, "relu")         # narrower than 2 x cin
