"""Latent frames that no step of a run wrote must not reach its audio.

The one-shot generator decodes every utterance of a batch over the longest one's frames.  The decoder is causal, but its window attention (attn_window.hip)
gives the keys of later frames weight zero instead of skipping them, and a 32-query tile spans two 16-row frames: a NaN in the frame behind an utterance's
last one turned that last frame into NaN whenever the last frame's index was even.  Such NaNs came from fresh device memory (seen when a test before the
first model of the process had freed NaN-filled buffers) and from an earlier request in the same slot whose own latents were NaN.  batch_reset now zeroes
the batch's latent frames."""
import numpy as np
import pytest

import test_gpu_dsp as TD
from test_gpu_dsp import tiny  # noqa: F401

pytestmark = pytest.mark.gpu


def test_nan_frames_of_an_earlier_request_do_not_reach_a_shorter_one_in_its_slot(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    toks = [[3, 7, 11], [4, 7, 12]]
    short = [TD._cfg(pkg, 3), TD._cfg(pkg, 12)]          # slot 0: 3 frames (the last one has index 2), beside 12
    before = gm.generate_batch(toks, short)
    assert [r.n_frames for r in before] == [3, 12] and all(np.isfinite(r.pcm).all() for r in before)
    bad = np.full((12, gm.info.ldim), np.nan, np.float32)   # a request whose own noise is NaN: its 12 latent frames are NaN, its neighbour's are not
    dirty = gm.generate_batch(toks, [TD._cfg(pkg, 12, noise=bad), TD._cfg(pkg, 12)])
    assert np.isnan(dirty[0].pcm).all() and np.isfinite(dirty[1].pcm).all()
    after = gm.generate_batch(toks, short)
    for a, b in zip(after, before):
        assert np.isfinite(a.pcm).all()
        assert a.n_frames == b.n_frames and np.array_equal(a.pcm.view(np.uint32), b.pcm.view(np.uint32))
