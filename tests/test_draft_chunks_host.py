"""Host side of drafting above the native row cap: draft_chunks() and the aic_lstm_max_rows export (no GPU needed)."""
import os
import re

import pytest

from arcticinference_amd import _native
from arcticinference_amd.speculator import draft_chunks, padding_size


@pytest.mark.parametrize("cap", [65, 128, 256])
def test_draft_chunks_are_even_and_complete(cap):
    for B in range(1, 4 * cap + 2):
        sizes = draft_chunks(B, cap)
        assert sum(sizes) == B
        assert all(0 < n <= cap for n in sizes)
        assert max(sizes) - min(sizes) <= 1
        if B <= cap:
            assert sizes == [B]
        else:
            # every chunk of a batch above the cap (any cap >= 65; the native one is 256) is wider than the fp8 head's
            # 32 rows: it takes the bf16 head, as the whole batch would (arctic_speculator.py:726-728)
            assert len(sizes) == -(-B // cap) and all(n > 32 for n in sizes), (B, sizes)


def test_draft_chunks_examples():
    assert draft_chunks(256, 256) == [256]
    assert draft_chunks(257, 256) == [129, 128]
    assert draft_chunks(300, 256) == [150, 150]
    assert draft_chunks(270, 256) == [135, 135]          # not [256, 14]: a 14-row remainder would take the fp8 head
    assert draft_chunks(padding_size(1000), 256) == [256, 256, 256, 256]
    assert draft_chunks(130, 64) == [44, 43, 43]


def test_max_rows_export_is_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arctic_hip.h")).read()
    assert re.search(r"\bint\s+aic_lstm_max_rows\s*\(\s*void\s*\)\s*;", hdr)
    assert "aic_lstm_max_rows" in _native.EXPORTED_SYMBOLS
    assert _native.lib().aic_lstm_max_rows() == 256
