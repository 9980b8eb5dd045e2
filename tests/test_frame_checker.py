"""CPU: the self-describing frame's numpy restatement (tests/frame_checker.py) does what the
definition in include/lora_mi355x.h says: the symbol counts, the round trip over the whole grid
of shapes, what the header's rounding and its Hamming 8/4 codewords absorb, every way a header
can be bad, the SHORT and CRC statuses and the zero padding of every output.  The device codec
is held to this checker as integers by tests/test_gpu_frame.py."""
import numpy as np
import pytest

from lora_phy_amd import codes
from tests import frame_checker as fc

SFS = range(7, 13)


def sizes(sf):
    return (0, 1, 2, 3, 4, 5, sf, 16, 17, 255)


def payload_of(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8).tobytes()


def test_symbol_counts():
    table = [(7, 1, 1, 0, 13), (7, 1, 1, 1, 13), (7, 1, 1, 16, 38), (7, 1, 1, 255, 378),
             (12, 4, 1, 0, 8), (12, 4, 1, 1, 16), (12, 4, 1, 16, 32), (12, 4, 1, 255, 352)]
    for sf, rdd, crc, n, nsym in table:
        assert fc.frame_symbols(sf, n, rdd, crc) == nsym, (sf, rdd, crc, n)


@pytest.mark.parametrize("sf", SFS)
def test_round_trip_over_the_grid(sf):
    """SF x rdd 0-4 x crc 0/1 x ten sizes: the encoded frame has the formula's length and its
    symbols fit sf bits, it decodes to its payload with status OK and no error, the payload's
    tail is zeros, and without its last symbol it is SHORT with a zero payload."""
    for rdd in range(5):
        for crc in (0, 1):
            for n in sizes(sf):
                key = (sf, rdd, crc, n)
                pay = payload_of(n, 1000 * sf + 100 * rdd + 10 * crc + n)
                sym = fc.encode_frame(pay, sf, rdd, crc)
                assert len(sym) == fc.frame_symbols(sf, n, rdd, crc), key
                assert int(sym.max()) < (1 << sf) and not (sym[:8] & 3).any(), key
                res = fc.decode_frame(sym, sf)
                assert [res[k] for k in fc.FIELDS] == [fc.OK, n, rdd, crc, len(sym), 0], key
                assert res["payload"][:n].tobytes() == pay and not res["payload"][n:].any(), key
                cut = fc.decode_frame(sym[:-1], sf)
                assert cut["status"] == fc.SHORT and not cut["payload"].any(), key
                if len(sym) > 8:  # the header is still whole: the fields are set
                    assert [cut[k] for k in fc.FIELDS[1:]] == [n, rdd, crc, len(sym), 0], key
                else:
                    assert [cut[k] for k in fc.FIELDS[1:]] == [0, 0, 0, 0, 0], key


@pytest.mark.parametrize("sf", SFS)
def test_header_absorbs_one_bin_on_every_symbol(sf):
    rng = np.random.default_rng(sf)
    for rdd in range(5):
        for crc in (0, 1):
            for n in sizes(sf):
                pay = payload_of(n, n + rdd)
                sym = fc.encode_frame(pay, sf, rdd, crc).astype(np.int64)
                for d in (np.ones(8, np.int64), -np.ones(8, np.int64), rng.choice([-1, 1], 8)):
                    off = sym.copy()
                    off[:8] = (off[:8] + d) % (1 << sf)
                    res = fc.decode_frame(off.astype(np.uint16), sf)
                    assert [res[k] for k in fc.FIELDS] == [fc.OK, n, rdd, crc, len(sym), 0], (sf, rdd, crc, n, d)
                    assert res["payload"][:n].tobytes() == pay


@pytest.mark.parametrize("sf", SFS)
def test_header_survives_one_wrong_symbol(sf):
    """One header symbol replaced by any other multiple of four bins is at most one bit per
    codeword of the block: Hamming 8/4 corrects it, for the header and the block's data alike.
    (Every value at SF 7-9; 48 drawn values per symbol above, the code does not depend on it.)"""
    rng = np.random.default_rng(100 + sf)
    values = np.arange(1 << (sf - 2)) << 2
    for rdd, crc, n in ((1, 1, 0), (4, 0, 3), (0, 1, 20), (2, 1, 17)):
        pay = payload_of(n, n)
        sym = fc.encode_frame(pay, sf, rdd, crc)
        for i in range(8):
            for v in (values if sf <= 9 else rng.choice(values, 48, replace=False)):
                if v == sym[i]:
                    continue
                bad = sym.copy()
                bad[i] = v
                res = fc.decode_frame(bad, sf)
                assert [res[k] for k in fc.FIELDS[:5]] == [fc.OK, n, rdd, crc, len(sym)], (sf, rdd, crc, n, i, v)
                assert res["payload"][:n].tobytes() == pay and res["errors"] <= sf - 2


def header_symbols(sf, nibbles, flip=None):
    """Eight header symbols from five header nibbles (the block's data codewords zero), with
    ``flip`` = (codeword, mask) XORed into a codeword."""
    cw = np.zeros(sf - 2, np.uint8)
    cw[:5] = codes.encode_hamming84(nibbles)
    if flip:
        cw[flip[0]] ^= flip[1]
    return codes.binary_to_gray16(codes.diagonal_interleave(cw, sf - 2, 4)).astype(np.uint16) << 2


@pytest.mark.parametrize("sf", SFS)
def test_each_way_a_header_is_bad(sf):
    good = fc.header_nibbles(9, 3, 1)
    bad_header = {"status": fc.HEADER, "nbytes": 0, "rdd": 0, "crc": 0, "nsym": 0, "errors": 0}
    assert fc.decode_header(header_symbols(sf, good), sf)["status"] == fc.OK
    # one flipped bit is corrected and counted, two in one codeword raise `bad`
    one = fc.decode_header(header_symbols(sf, good, (2, 0x10)), sf)
    assert (one["status"], one["nbytes"], one["rdd"], one["crc"], one["errors"]) == (fc.OK, 9, 3, 1, 1)
    for j in range(5):
        assert fc.decode_header(header_symbols(sf, good, (j, 0x41)), sf) == bad_header, j
    # nibble 3 holds one bit of the 5-bit checksum
    assert fc.decode_header(header_symbols(sf, good[:3] + [good[3] | 2, good[4]]), sf) == bad_header
    # a checksum that is not the fields'
    assert fc.decode_header(header_symbols(sf, good[:4] + [good[4] ^ 1]), sf) == bad_header
    assert fc.decode_header(header_symbols(sf, [good[0], good[1] ^ 8] + good[2:]), sf) == bad_header
    # rdd 5..7 with the right checksum
    for rdd in (5, 6, 7):
        h1 = (rdd << 1) | 1
        h2 = codes.header_checksum([9, h1])
        assert fc.decode_header(header_symbols(sf, [0, 9, h1, h2 >> 4, h2 & 15]), sf) == bad_header, rdd
    # the full decode of a bad header: a zero payload
    res = fc.decode_frame(header_symbols(sf, good[:4] + [good[4] ^ 1]), sf, max_bytes=7)
    assert res["status"] == fc.HEADER and res["payload"].shape == (7,) and not res["payload"].any()


def test_short_statuses_and_avail():
    sf, pay = 8, payload_of(20, 5)
    sym = fc.encode_frame(pay, sf, 2, 1)
    none = [fc.SHORT, 0, 0, 0, 0, 0]
    for avail in (-3, 0, 7):
        assert [fc.decode_frame(sym, sf, avail)[k] for k in fc.FIELDS] == none
        assert [fc.decode_header(sym, sf, avail)[k] for k in fc.FIELDS] == none
    assert [fc.decode_header(sym[:7], sf)[k] for k in fc.FIELDS] == none
    # header-only mode is SHORT for avail < 8 alone
    assert fc.decode_header(sym, sf, 8) == fc.decode_header(sym, sf) == {
        "status": fc.OK, "nbytes": 20, "rdd": 2, "crc": 1, "nsym": len(sym), "errors": 0}
    for avail in (8, len(sym) - 1):
        res = fc.decode_frame(sym, sf, avail)
        assert [res[k] for k in fc.FIELDS] == [fc.SHORT, 20, 2, 1, len(sym), 0] and not res["payload"].any()
    for avail in (len(sym), len(sym) + 9):  # avail is clamped to the symbols given
        assert fc.decode_frame(sym, sf, avail)["status"] == fc.OK
    # symbols after the frame's own are not the frame's
    longer = np.concatenate([sym, np.full(11, 0xFFFF, np.uint16)])
    res = fc.decode_frame(longer, sf)
    assert res["status"] == fc.OK and res["payload"][:20].tobytes() == pay
    # a payload buffer narrower than the frame's bytes
    res = fc.decode_frame(sym, sf, max_bytes=19)
    assert [res[k] for k in fc.FIELDS] == [fc.SHORT, 20, 2, 1, len(sym), 0] and not res["payload"].any()


@pytest.mark.parametrize("sf", (7, 10, 12))
def test_crc_status(sf):
    """At rate 4/4 nothing corrects a flipped data bit: the checksum is what notices, in a
    payload byte and in the checksum's own bytes; the payload is written all the same.  Without
    the CRC flag the same frame is OK."""
    n = 12
    pay = payload_of(n, sf)
    for where in (0, 2 * n - 1, 2 * n, 2 * n + 3):  # a data nibble: first, last, and the checksum's
        sym = fc.encode_frame(pay, sf, 0, 1)
        nh = sf - 7
        if where < nh:  # that nibble rides in block 0, under Hamming 8/4
            continue
        c = where - nh
        blk, row = divmod(c, sf)
        # bit 0 of codeword `row` of the block is bit `row` of the block's symbol 0
        s = 8 + blk * 4
        sym[s] = codes.binary_to_gray16(codes.gray_to_binary16(sym[s]) ^ (1 << row))
        res = fc.decode_frame(sym, sf)
        assert res["status"] == fc.CRC and res["nbytes"] == n and res["errors"] == 0, (sf, where)
        got = res["payload"][:n].tobytes()
        if where < 2 * n:
            assert got != pay and sum(bin(a ^ b).count("1") for a, b in zip(got, pay)) == 1
        else:
            assert got == pay
    sym = fc.encode_frame(pay, sf, 0, 0)
    s = 8
    sym[s] = codes.binary_to_gray16(codes.gray_to_binary16(sym[s]) ^ 1)
    res = fc.decode_frame(sym, sf)
    assert res["status"] == fc.OK and res["payload"][:n].tobytes() != pay


@pytest.mark.parametrize("sf", SFS)
def test_an_empty_payload(sf):
    for rdd in range(5):
        bare = fc.encode_frame(b"", sf, rdd, 0)
        assert len(bare) == 8
        res = fc.decode_frame(bare, sf)
        assert [res[k] for k in fc.FIELDS] == [fc.OK, 0, rdd, 0, 8, 0] and not res["payload"].any()
        sym = fc.encode_frame(b"", sf, rdd, 1)  # four nibbles of checksum, sf - 7 of them in block 0
        assert len(sym) == (8 if sf >= 11 else 8 + 4 + rdd)
        res = fc.decode_frame(sym, sf)
        assert [res[k] for k in fc.FIELDS] == [fc.OK, 0, rdd, 1, len(sym), 0]
    assert fc.data_bytes(b"", 1) == bytes([codes.sx1272_data_checksum(b"") & 0xFF,
                                           codes.sx1272_data_checksum(b"") >> 8])


def test_the_checksum_covers_the_whole_payload():
    pay = payload_of(9, 1)
    c = codes.sx1272_data_checksum(pay)
    assert fc.data_bytes(pay, 1) == pay + bytes([c & 0xFF, c >> 8]) and fc.data_bytes(pay, 0) == pay
    assert c != codes.sx1272_data_checksum(pay[2:])  # not the library chain's window


def test_batches_are_zero_padded():
    sf, rdd, crc = 9, 3, 1
    nbytes = np.array([0, 30, 7, 1])
    pay = np.random.default_rng(3).integers(0, 256, (4, 30)).astype(np.uint8)
    sym, nsym = fc.encode_batch(pay, nbytes, sf, rdd, crc)
    assert sym.shape == (4, fc.frame_symbols(sf, 30, rdd, crc))
    for f in range(4):
        assert nsym[f] == fc.frame_symbols(sf, nbytes[f], rdd, crc) and not sym[f, nsym[f]:].any()
    res = fc.decode_batch(sym, sf, max_bytes=40)
    assert (res["status"] == fc.OK).all() and np.array_equal(res["nbytes"], nbytes)
    for f in range(4):
        assert np.array_equal(res["payload"][f, :nbytes[f]], pay[f, :nbytes[f]])
        assert not res["payload"][f, nbytes[f]:].any()
    head = fc.decode_batch(sym, sf)
    assert "payload" not in head and all(np.array_equal(head[k], res[k]) for k in fc.FIELDS)


def test_gather_host():
    flat = np.arange(1, 21).astype(np.complex64)
    got = fc.gather_host(flat, [0, 3, 17, 18, -1, 20, 5], [4, 0, 3, 9, 4, 2, -2], 5)
    want = np.zeros((7, 5), np.complex64)
    want[0, :4] = flat[:4]
    want[2, :3] = flat[17:]
    want[3, :2] = flat[18:]
    assert np.array_equal(got, want)
    assert np.array_equal(fc.gather_host(flat, [2], [9], 4), flat[None, 2:6])  # clamped to the cut


# ---------------------------------------------------------------------------------
# The candidate list and the pass over decoded headers
# ---------------------------------------------------------------------------------
def test_selection_rule_on_hand_made_slots():
    step, row_len = 128, 20000
    OK, BAD = fc.OK, fc.HEADER

    def select(slots, first=0, max_symbols=40, row_len=row_len):
        s, n, end = fc.select_frames_host([x[0] for x in slots], [x[1] for x in slots], [x[2] for x in slots], step,
                                          row_len, max_symbols, first)
        return list(s), list(n), end

    # a bad header between two good ones
    assert select([(100, OK, 8), (1500, BAD, 0), (3000, OK, 13)]) == ([100, 3000], [8, 13], 3000 + 15 * step)
    # a candidate inside an accepted frame, its header good by chance: it starts before `first`
    assert select([(100, OK, 13), (100 + 5 * step, OK, 8), (100 + 15 * step, OK, 8)]) == (
        [100, 100 + 15 * step], [13, 8], 100 + 25 * step)
    # a frame that runs over the row's end, and one that ends exactly on it
    assert select([(row_len - 10 * step + 1, OK, 8)]) == ([], [], 0)
    assert select([(row_len - 10 * step, OK, 8)]) == ([row_len - 10 * step], [8], row_len)
    # a header stating more symbols than the caller takes
    assert select([(0, OK, 41), (0, OK, 40)]) == ([0], [40], 42 * step)
    # statuses other than OK, an empty slot
    assert select([(0, fc.SHORT, 8), (0, fc.CRC, 8), (-1, OK, 8), (50, OK, 8)]) == ([50], [8], 50 + 10 * step)
    # first: nothing before it, and it is the end when nothing is accepted
    assert select([(100, OK, 8), (3000, OK, 8)], first=101) == ([3000], [8], 3000 + 10 * step)
    assert select([(100, OK, 8)], first=5000) == ([], [], 5000)
    # capacity below the count: the count stays, the slots hold the first ones, then -1 / 0
    s, n, end = fc.select_frames_host([100, 3000, 6000], [OK] * 3, [8, 13, 8], step, row_len, 40)
    assert len(s) == 3 and end == 6000 + 10 * step
    assert fc.to_slots(s, 2, -1, np.int64).tolist() == [100, 3000] and fc.to_slots(n, 2, 0, np.int32).tolist() == [8, 13]
    assert fc.to_slots(s, 5, -1, np.int64).tolist() == [100, 3000, 6000, -1, -1]
    assert fc.to_slots(n, 5, 0, np.int32).tolist() == [8, 13, 8, 0, 0] and fc.to_slots(s, 0, -1, np.int64).shape == (0,)
    # first per row: each row's pass is its own
    rows = [select([(100, OK, 8), (3000, OK, 8)], first=f) for f in (0, 101, 3001)]
    assert [r[0] for r in rows] == [[100, 3000], [3000], []] and [r[2] for r in rows] == [3000 + 10 * step] * 2 + [3001]
    # slot order, not start order, decides
    assert select([(3000, OK, 8), (100, OK, 8)]) == ([3000], [8], 3000 + 10 * step)


def test_candidate_list_against_the_fixed_length_finder():
    """Every start the fixed-length finder accepts (frames of 8 symbols: the header's length) is
    among the listed candidates, the list has no equal neighbours, and every entry fits the row."""
    from tests import scan_checker as sc

    sf, osr, k = 7, 1, 4
    step = (1 << sf) * osr
    hop = step // k
    for seed in range(4):
        m = fc.synthetic_scan(seed, sf, k, 3000, 0.3)
        row_len = 2999 * hop + step - 77 * seed
        c = fc.find_candidates_host(m, hop, sf, osr, row_len=row_len)
        assert len(c) > 50 and (c >= 0).all() and (c + 10 * step <= row_len).all() and (np.diff(c) != 0).all()
        fixed = sc.find_frames_host(m, hop, sf, osr, 8, row_len=row_len)
        assert len(fixed) > 3 and set(fixed) <= set(c)
        # all good headers of 8 symbols: the pass over the list is the fixed-length finder
        s, n, end = fc.select_frames_host(c, [fc.OK] * len(c), [8] * len(c), step, row_len, 8)
        assert np.array_equal(s, fixed) and end == fixed[-1] + 10 * step
    none = fc.find_candidates_host({"index": np.zeros(3, np.uint16), "power": np.zeros(3, np.float32),
                                    "power_avg": np.zeros(3, np.float32)}, hop, sf, osr)
    assert none.shape == (0,) and none.dtype == np.int64
