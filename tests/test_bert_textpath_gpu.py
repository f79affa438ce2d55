"""BERT through the refactored text calls: vr_query_text, vr_query_text_batch and vr_rerank_text now reach the
WordPiece tokenizer through the engine's tokenizer interface. The same seeded run (tests/bert_textpath_case.py) must
give, bit for bit, what the engine gave before that change (tests/golden/textpath_bert.npz, recorded with it)."""
import os

import numpy as np
import pytest

import bert_textpath_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textpath_bert.npz")


def test_bert_text_calls_are_unchanged(gpu):
    want = np.load(GOLDEN)
    got = bert_textpath_case.run()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert want["batch_hybrid"].any() and not want["batch_hybrid"].all()
