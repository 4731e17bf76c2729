"""parity.compare_frame, the one comparison every GPU parity test goes through, pinned on the CPU with stand-in
renderers over numpy arrays: 4 x 3-pixel planes (0: RGBA16F, 1: f32, 12: raw) and reservoir buffers of 64-byte records
(words 0, 1, 14, 15 f16 pairs, 4..11 f32, the rest raw: random is words 2, 3)."""
import numpy as np
import pytest

from parity import canon_frame, compare_frame

F16_NANS, F32_NANS = (0x7C01, 0xFE00), (0x7F800001, 0xFFC12345)  # two payloads each


class Standin:
    """output(oid), reservoirs(rid) and counters() over arrays; only the listed ids exist."""

    def __init__(self, records=12, outputs=range(17), rids=range(10), seed=1):
        rng = np.random.default_rng(seed)  # exponent bits cleared below: finite values, no NaN by accident
        self.planes = {oid: rng.integers(0, 256, (3, 4, 8), np.uint8) & 0x3F for oid in outputs}
        self.res = {rid: rng.integers(0, 1 << 32, (records, 16), np.uint64).astype(np.uint32) & np.uint32(0x3F3F3F3F)
                    for rid in rids}

    def output(self, oid):
        return self.planes[oid]

    def reservoirs(self, rid):
        return self.res[rid]

    def counters(self):
        return {"primary": 12}


def errors_of(r, ref, **kw):
    errors = []
    compare_frame(r, ref, 3, errors, **kw)
    return errors


def test_identical_inputs_give_no_errors():
    r, o = Standin(), Standin()
    assert errors_of(r, o) == [] and errors_of(r, canon_frame(o)) == []


@pytest.mark.parametrize("stored", [False, True], ids=["live", "stored"])
def test_one_flipped_bit_gives_one_error_naming_frame_and_id(stored):
    for kind, key, label in (("planes", 0, "frame 3 output 0:"), ("planes", 1, "frame 3 output 1:"),
                             ("planes", 12, "frame 3 output 12:"), ("res", 7, "frame 3 reservoir 7:")):
        r, o = Standin(), Standin()
        getattr(r, kind)[key].reshape(-1)[5] ^= 4
        errors = errors_of(r, canon_frame(o) if stored else o)
        assert len(errors) == 1 and errors[0].startswith(label), errors


def test_nan_payloads_compare_equal_where_the_format_has_nans():
    r, o = Standin(), Standin()
    for x, f16, f32 in ((r, F16_NANS[0], F32_NANS[0]), (o, F16_NANS[1], F32_NANS[1])):
        x.planes[0].view(np.uint16)[1, 2, 3] = f16
        x.planes[1].view(np.uint32)[2, 1, 0] = f32
        for word in (0, 1, 14, 15):
            x.res[2][3, word] = f16 | (f16 << 16)
        x.res[2][3, 4:12] = f32
    assert errors_of(r, o) == []
    for word in (2, 3):  # random is compared raw: the same two patterns there differ
        r, o = Standin(), Standin()
        r.res[2][3, word], o.res[2][3, word] = F16_NANS
        errors = errors_of(r, o)
        assert len(errors) == 1 and errors[0].startswith("frame 3 reservoir 2:"), errors
    r, o = Standin(), Standin()  # and a raw plane keeps its payloads
    r.planes[12].view(np.uint32)[0, 0, 0], o.planes[12].view(np.uint32)[0, 0, 0] = F32_NANS
    assert len(errors_of(r, o)) == 1


@pytest.mark.parametrize("stored", [False, True], ids=["live", "stored"])
def test_longer_reference_buffers_compare_their_prefix(stored):
    r, o = Standin(records=12), Standin(records=12)
    tail = Standin(records=8, seed=2)
    o.res = {rid: np.concatenate([o.res[rid], tail.res[rid]]) for rid in range(10)}  # 20 records: a prefix and a tail
    o.res[4][15, 6] ^= 1  # in the tail (as all of it): ignored
    assert errors_of(r, canon_frame(o) if stored else o) == []
    o.res[4][11, 6] ^= 1  # the last record of the prefix
    errors = errors_of(r, canon_frame(o) if stored else o)
    assert len(errors) == 1 and errors[0].startswith("frame 3 reservoir 4:"), errors


def test_racy_tolerance_applies_to_the_listed_ids_only():
    r, o = Standin(records=100), Standin(records=100)
    for rec in (10, 50, 99):
        r.res[5][rec, 8] ^= 1
    stats = []
    assert errors_of(r, o, racy=(5,), stats=stats) == [] and stats == [(3, 5, 97 / 100)]
    errors = errors_of(r, o, racy=(4,))  # the same three records on an id that is not listed
    assert len(errors) == 1 and errors[0].startswith("frame 3 reservoir 5:"), errors
    assert len(errors_of(r, o)) == 1  # the default is exact everywhere
    r.res[5][60, 8] ^= 1  # a fourth record: 0.96
    errors = errors_of(r, o, racy=(5,), stats=stats)
    assert errors == ["frame 3 reservoir 5: only 0.9600 of records exact"] and stats[-1] == (3, 5, 96 / 100)


def test_outputs_and_rids_restrict_what_is_read():
    r, o = Standin(outputs=(10, 15), rids=(3,)), Standin(outputs=(10, 15), rids=(3,))
    assert errors_of(r, o, outputs=(10, 15), rids=[3]) == []
    assert errors_of(r, o, outputs=(), rids=()) == []
    with pytest.raises(KeyError):  # the stand-ins raise on any other id
        errors_of(r, o, outputs=(10, 11), rids=[3])
    with pytest.raises(KeyError):
        errors_of(r, o, outputs=(10,), rids=[3, 4])
