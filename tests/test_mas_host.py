"""CPU: the restated alignment search (tests/mas_ref.py) on cases worked out by hand, its structural properties, and the public
surface forward() / maximum_path() need (signature and module: no GPU touched)."""
import inspect

import numpy as np
import pytest

import mas_ref


def run(v, t_x=None, t_y=None):
    v = np.asarray(v, dtype=np.float32)
    t_x = v.shape[0] if t_x is None else t_x
    t_y = v.shape[1] if t_y is None else t_y
    return mas_ref.maximum_path_each(v.copy(), t_x, t_y)


def test_two_by_three_by_hand():
    """token 0 takes frames 0 .. k, token 1 the rest: k = 0 scores -1 - 2 - 1 = -4, k = 1 scores -1 - 1 - 1 = -3"""
    p = run([[-1, -1, -5], [-9, -2, -1]])
    assert p.tolist() == [[1, 1, 0], [0, 0, 1]]
    # ... and with frame 1 cheaper on token 1: k = 0 scores -1 - 0.5 - 1 = -2.5, k = 1 still -3
    p = run([[-1, -1, -5], [-9, -0.5, -1]])
    assert p.tolist() == [[1, 0, 0], [0, 1, 1]]


def test_three_by_three_is_the_diagonal():
    """as many frames as tokens: one frame each, whatever the scores say"""
    p = run([[-5, 0, 0], [0, -7, 0], [0, 0, -9]])
    assert p.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


def test_three_by_four_by_hand():
    """one spare frame: the doubled token is 0, 1 or 2.  Scores: doubled 0: a00 + a01 + a12 + a23 = -1 - 4 - 1 - 1 = -7; doubled 1:
    a00 + a11 + a12 + a23 = -1 - 1 - 1 - 1 = -4; doubled 2: a00 + a11 + a22 + a23 = -1 - 1 - 3 - 1 = -6"""
    p = run([[-1, -4, 0, 0], [0, -1, -1, 0], [0, 0, -3, -1]])
    assert p.tolist() == [[1, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 1]]


def test_tie_stays_on_the_same_token():
    """all scores equal: walking back from the last frame the comparison `<` is strict, so the path stays on the last token until
    the diagonal forces it down -- equal scores stay on the same token"""
    assert run(np.zeros((2, 3))).tolist() == [[1, 0, 0], [0, 1, 1]]
    assert run(np.zeros((3, 6))).tolist() == [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1]]


def test_padding_is_never_read():
    v = np.full((4, 7), np.nan, dtype=np.float32)
    v[:2, :3] = [[-1, -1, -5], [-9, -2, -1]]
    p = mas_ref.maximum_path_each(v, 2, 3)
    assert p[:2, :3].tolist() == [[1, 1, 0], [0, 0, 1]] and p.sum() == 3


@pytest.mark.parametrize("kind", ["gauss", "ties"])
def test_path_properties(kind):
    rng = np.random.default_rng(3)
    for t_x, t_y in [(1, 1), (1, 5), (2, 2), (2, 3), (7, 7), (7, 8), (7, 17), (33, 70), (64, 65)]:
        v = (rng.normal(-150.0, 20.0, (t_x + 2, t_y + 3)) if kind == "gauss" else rng.integers(-3, 1, (t_x + 2, t_y + 3))).astype(np.float32)
        p = mas_ref.maximum_path_each(v.copy(), t_x, t_y)
        mas_ref.check_path(p, t_x, t_y)
        # the path the search returns scores at least as well as the two extreme paths (first / last token takes the spare frames)
        score = lambda idx: float(sum(np.float64(v[idx[y], y]) for y in range(t_y)))
        got = p[:t_x, :t_y].argmax(axis=0)
        first = np.minimum(np.maximum(np.arange(t_y) - (t_y - t_x), 0), t_x - 1)
        last = np.minimum(np.arange(t_y), t_x - 1)
        assert score(got) >= max(score(first), score(last)) - 1e-2


def test_batch_wrapper_outputs():
    rng = np.random.default_rng(5)
    v = rng.normal(-150.0, 20.0, (2, 5, 9)).astype(np.float32)
    keep = v.copy()
    paths, fi, dur = mas_ref.maximum_path(v, [5, 3], [9, 4])
    assert np.array_equal(v, keep)
    assert fi[1, 4:].tolist() == [-1] * 5 and dur[1].tolist()[3:] == [0, 0] and dur.sum(axis=1).tolist() == [9, 4]
    for b, (t_x, t_y) in enumerate([(5, 9), (3, 4)]):
        mas_ref.check_path(paths[b], t_x, t_y)
        assert all(paths[b, fi[b, y], y] == 1 for y in range(t_y))


def test_forward_has_the_reference_signature():
    from jyutvoice_amd.models.jyutvoice_tts import JyutVoiceTTS
    params = inspect.signature(JyutVoiceTTS.forward).parameters
    names = list(params)
    assert names[:11] == ["self", "x", "x_lengths", "y", "y_lengths", "lang", "tone", "word_pos", "syllable_pos", "spk_embed", "decoder_h"]
    for extra in ("t", "z", "cfg_mask", "cond_index", "generator", "return_parts"):
        assert params[extra].kind is inspect.Parameter.KEYWORD_ONLY


def test_maximum_path_module_exists():
    from jyutvoice_amd.utils import monotonic_align
    assert list(inspect.signature(monotonic_align.maximum_path).parameters) == ["value", "mask"]
