"""The pole layers without padding traffic and their composite in one pass per eye (render_kernels.hip: k_composite_poles_v4,
launch_pole_finish over the layer's own rows), against the oracle byte for byte. The cases are tests/composite_cases.py's."""
import pytest

import composite_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return tmp_path_factory.mktemp("rig_composite")


@pytest.fixture(scope="module")
def rig_path(tmpdir, rig_json, s360lib):
    return S.make_rig(rig_json, tmpdir)


def _both_cover_some_rows(t, b, h):
    assert t + b > h and t < h and b < h, (t, b, h)  # rows with both layers, rows with one


def test_both_poles_two_frames(rig_path, oracle):
    """(a), (e): both poles; a second frame of other content in the same context has all-zero padding rows again."""
    S.check_against_oracle(rig_path, oracle, S.flags(), yaws=(0.0, 2.3), expect_rows=_both_cover_some_rows)


@pytest.mark.parametrize("which", ["enable_top", "enable_bottom"])
def test_one_pole_only(rig_path, oracle, which):
    """(b): the other layer is absent, which is not a layer of transparent rows."""
    S.check_against_oracle(rig_path, oracle, S.flags(**dict(dict(enable_top=0, enable_bottom=0), **{which: 1})))


def test_masks_fused_against_per_layer(rig_path, tmpdir):
    """(c): pole_units(mask) + composite(mask) for every single unit, each eye's pair and all four."""
    S.check_masks_against_per_layer_path(rig_path, tmpdir)


def test_width_no_multiple_of_4_takes_the_per_layer_path(rig_path, oracle):
    """(d): 14 x 71 (x 35 at a quarter of the size) columns."""
    w = S.P * ((S.EQR_W // S.P) - 1)
    assert w % 4 != 0
    S.check_against_oracle(rig_path, oracle, S.flags(eqr_width=w))


def test_three_slots_in_one_batch(rig_path):
    """(f)"""
    S.check_batch(rig_path, 3)


def test_rows_no_layer_covers(tmpdir, rig_json, oracle, s360lib):
    """(g): pole cameras of 1.2 rad: top_rows + bottom_rows < H, the rows between take t = 0 twice."""
    def rows(t, b, h):
        assert 0 < t and 0 < b and t + b < h, (t, b, h)
    S.check_against_oracle(S.make_rig(rig_json, tmpdir, pole_fov=1.2), oracle, S.flags(), expect_rows=rows)
