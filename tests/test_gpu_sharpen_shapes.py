"""sharpen (iirLowPass + sharpenWithIirLowPass, Filter.h:40-127) against the oracle byte for byte at the shapes where the IIR
passes change path — they keep no float image: the anticausal half makes the causal values again tile by tile from saved chain
states — and the batched frame whose final resize only changes the width. The cases are tests/sharpen_shapes_cases.py's."""
import pytest

import sharpen_shapes_cases as S
from surround360_amd import render as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig_path(tmp_path_factory, rig_json, s360lib):
    return S.make_rig(rig_json, tmp_path_factory.mktemp("rig_sharpen"))


@pytest.fixture(scope="module")
def ctx(rig_path):
    c = R.Context(R.RigDescription(rig_path), R.make_params(**S.frame_flags()))
    yield c
    c.close()


@pytest.mark.parametrize("content", S.CONTENTS)
@pytest.mark.parametrize("h,w", S.SHAPES)
def test_sharpen_shape(ctx, oracle, h, w, content):
    S.check_shape(ctx, oracle, h, w, content)


def test_batch_sharpened_width_only_resize(rig_path, oracle):
    """Three slots, sharpening 0.25, 1008x504 eyes resized to 957x504 each: slot by slot the frame rendered alone, and slot 0
    the oracle's frame."""
    S.check_batch(rig_path, 3, oracle)


def test_batch_sharpened_ragged_last_group(rig_path):
    """One slot more than a set of sharpen launches holds: the last group is a single slot's eyes."""
    S.check_batch(rig_path, S.GROUP_SLOTS + 1)
