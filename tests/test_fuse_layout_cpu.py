"""The fusion's LDS layout without a GPU, through the refusal fuse_impl answers with before any device work: the byte count and the
capacity it prints must be what the per-row formula of the commit before the layout was stated once gives (frozen text below), for every
mode that changes the layout and for K = 1, 3 and 62, at max_rows = 2048 and at the first max_rows that is refused."""
import ctypes
import re

import pytest

ONE = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below is refused before the launch
LDS, STATIC, SLACK = 160 * 1024, 512, 16

#        name               entry point                      score_mode  logp pool pres
MODES = [("probEn", "pe_proben_fuse_batch", 0, 0, 0, 0),
         ("avg", "pe_proben_fuse_batch", 1, 0, 0, 0),
         ("probEn_binary", "pe_proben_fuse_batch", 3, 0, 0, 0),
         ("logp", "pe_proben_fuse_batch_logp", None, 1, 0, 0),
         ("logp+pool", "pe_proben_fuse_batch_pooled", None, 1, 1, 0),
         ("logp+pres", "pe_proben_fuse_batch_presence", None, 1, 0, 1),
         ("logp+pool+pres", "pe_proben_fuse_batch_presence", None, 1, 1, 1)]


def per_row(K, score_mode, logp, pool, pres):
    """The parent's formula, frozen: bytes of LDS per row."""
    L = K + 1 if logp or score_mode == 0 else 2 if score_mode == 3 else 0
    return 8 * (6 + L + 5 + pool) + 4 + 4 + 4 * pres + 4 * 2 + 1


def call(entry, K, max_rows, score_mode, pool):
    from proben_amd import _lib
    wide = entry != "pe_proben_fuse_batch" and entry != "pe_proben_fuse_batch_logp"
    args = [ONE] * 5 + ([ONE] if wide else []) + [ONE, None, None, 1, K, max_rows] + ([] if score_mode is None else [score_mode])
    args += [0, 0.5, 640.0, 512.0] + ([None] if score_mode is None else []) + ([ONE if pool else None] if wide else [])
    args += ([ONE] if entry.endswith("presence") else []) + ([2] if wide else []) + [ONE] * 5 + ([None] if wide else [])
    args += [None] * 3 if entry.endswith(("posterior", "presence")) else []
    args += [None] if entry.endswith("presence") else []
    L = _lib.lib()
    return getattr(L, entry)(*args, None), L.pe_last_error().decode()


@pytest.mark.parametrize("K", [1, 3, 62])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_the_refusal_prints_the_parents_bytes_and_capacity(mode, K):
    name, entry, score_mode, logp, pool, pres = mode
    row = per_row(K, score_mode, logp, pool, pres)
    capacity = (LDS - STATIC - SLACK) // row
    first = next(m for m in range(1, 2049) if ((m + 1) & ~1) * row + SLACK + STATIC > LDS)
    assert capacity <= first <= capacity + 1
    for max_rows in (2048, first):
        status, err = call(entry, K, max_rows, score_mode, pool)
        assert status == -2, (name, K, max_rows, status, err)           # PE_ERR_UNSUPPORTED
        got = re.fullmatch(entry + r": (\d+) bytes of LDS needed \(> 160 KiB\): max_rows_per_image (\d+) is above the per-image capacity "
                           r"of (\d+) rows for this score mode / class count", err)
        assert got, err
        assert [int(x) for x in got.groups()] == [((max_rows + 1) & ~1) * row + SLACK + STATIC, max_rows, capacity], (name, K, err)
