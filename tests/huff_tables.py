"""Huffman table SHAPES for the device entropy decoder's tests: named families of valid tables that are not Annex K's,
each as the 4-tuple synth.encode_jpeg(huffman=...) takes -- DC luma, AC luma, DC chroma, AC chroma, each
(BITS[16], HUFFVAL).  What depends on a table's shape in jb_huff_core.h / jb_huff.hip -- the split between the 10-bit
first level and the 6-bit second level, the pool of 24 second-level tables a set shares, the widest symbol (a 16-bit
DC code + 11 magnitude bits), how fast lanes fall into step -- is reached only through tables like these.

Every family holds the whole alphabet the decoders accept (AC: EOB, ZRL, run 0..15 x size 1..10 = 162 symbols; DC:
0..11), so the project's writer can code any baseline content with it; every table is checked here: sum(BITS) ==
len(HUFFVAL), no symbol twice, Kraft sum <= 1.  t2_tables() counts the second-level tables a set needs the way the
format defines them (distinct 10-bit prefixes of the codes longer than 10 bits), without looking at the decoder.

Also here: the contents the tests code with these tables, a small bit writer for streams the project's writer cannot
make (hand_streams), and the child process that asks the genuine reference (python huff_tables.py --ref-dump files...)."""
import os
import sys

import numpy as np

T1_BITS = 10      # first-level lookup bits of the device decoder (jb_huff.h kJbT1Bits)
POOL = 24         # second-level tables a table set can hold (kJbT2Tables)

DC_SYMS = list(range(12))
AC_SYMS = [0x00, 0xf0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


def _synth():
    from jpeg_decoder_amd import synth
    return synth


def lengths_of(bits):
    """BITS -> the code length of every symbol, in HUFFVAL order."""
    return [ln for ln in range(1, 17) for _ in range(bits[ln - 1])]


def kraft(bits):
    """Kraft sum of a table in units of 2^-16 (65536 = complete)."""
    return sum(n << (16 - ln) for ln, n in enumerate(bits, 1))


def codes_of(bits):
    """Canonical codes (ITU-T T.81 Annex C): [(length, code)] in HUFFVAL order."""
    out, code = [], 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out.append((ln, code))
            code += 1
        code <<= 1
    return out


def table(pairs, alphabet):
    """[(symbol, length)] -> (BITS, HUFFVAL): sorted by length, the given order kept within a length."""
    pairs = sorted(pairs, key=lambda p: p[1])  # (stable)
    bits = [0] * 16
    for _, ln in pairs:
        assert 1 <= ln <= 16
        bits[ln - 1] += 1
    vals = [s for s, _ in pairs]
    check_table((bits, vals), alphabet)
    return bits, vals


def check_table(t, alphabet=None):
    bits, vals = t
    assert len(bits) == 16 and sum(bits) == len(vals), "BITS does not match HUFFVAL"
    assert len(set(vals)) == len(vals), "a symbol twice"
    assert kraft(bits) <= 1 << 16, "Kraft sum above 1"
    assert all(n <= 255 for n in bits)
    if alphabet is not None:
        assert set(alphabet) <= set(vals), "the alphabet is not covered"


def t2_prefixes(t):
    """The distinct first-level prefixes of a table's codes longer than the first level: one second-level table each."""
    return sorted({code >> (ln - T1_BITS) for ln, code in codes_of(t[0]) if ln > T1_BITS})


def t2_tables(tables):
    """Second-level tables a set of tables needs together (the pool is per set, not per table)."""
    return sum(len(t2_prefixes(t)) for t in tables)


def _by_counts(order, counts, alphabet):
    """symbols in `order`, the first counts[l0] of them at the shortest length l0, and so on."""
    lens = [ln for ln in sorted(counts) for _ in range(counts[ln])]
    assert len(lens) == len(order)
    return table(list(zip(order, lens)), alphabet)


# ---- the families ---------------------------------------------------------------------------------------------------
def annexk_reversed():
    """Annex-K BITS with HUFFVAL reversed: the most frequent symbols get the 16-bit codes."""
    return tuple((list(b), list(reversed(v))) for b, v in _synth().ANNEX_K_HUFFMAN)


def flat():
    """Every DC code 4 bits, every AC code 8 bits: under dense content every symbol has one width."""
    dc = _by_counts(DC_SYMS, {4: 12}, DC_SYMS)
    ac = _by_counts(AC_SYMS, {8: 162}, AC_SYMS)
    return dc, ac, dc, ac


def complete_allones():
    """Kraft sum exactly 1: the last code of every table is all ones."""
    s = _synth()
    dc = _by_counts(DC_SYMS, {3: 4, 4: 8}, DC_SYMS)
    assert kraft(dc[0]) == 1 << 16
    out = []
    for vals in (s.ANNEX_K_HUFFMAN[1][1], s.ANNEX_K_HUFFMAN[3][1]):
        ac = _by_counts(list(vals), {7: 94, 8: 68}, AC_SYMS)
        assert kraft(ac[0]) == 1 << 16 and codes_of(ac[0])[-1] == (8, 0xff)
        out.append(ac)
    return dc, out[0], dc, out[1]


def all16():
    """One short code (1 bit in the luma tables, 2 bits in the chroma tables), every other code 16 bits: DC size 11
    (27 bits a symbol) and the AC size-10 symbols (26 bits) are among the long ones."""
    def one_short(alphabet, short_sym, short_len):
        rest = [s for s in reversed(alphabet) if s != short_sym]
        return table([(short_sym, short_len)] + [(s, 16) for s in rest], alphabet)
    return (one_short(DC_SYMS, 0, 1), one_short(AC_SYMS, 0x00, 1), one_short(DC_SYMS, 1, 2), one_short(AC_SYMS, 0x01, 2))


def unary_dc_long():
    """DC: lengths 1..11 and one 16-bit code (size 11 in luma: the widest symbol there is; chroma counts the sizes
    down, so its size 11 has the 1-bit code and size 0 the 16-bit one); Annex-K AC."""
    s = _synth()
    lens = list(range(1, 12)) + [16]
    return (table(list(zip(DC_SYMS, lens)), DC_SYMS), s.ANNEX_K_HUFFMAN[1],
            table(list(zip(reversed(DC_SYMS), lens)), DC_SYMS), s.ANNEX_K_HUFFMAN[3])


def t1_split():
    """Codes on both sides of the first level's edge: AC tables with codes of 9, 10, 11 and 12 bits, given to the most
    frequent symbols in turn (EOB 9, 0x01 10, 0x02 11, 0x03 12, ...), the rarest 18 symbols on short codes; DC tables
    with 9, 10 and 11 bits.  The chroma AC table has an odd number of 11-bit codes, so one second-level table holds an
    11-bit code beside 12-bit ones."""
    s = _synth()

    def ac(vals, n9, n10, n11, n12):
        short = {4: 8, 5: 4, 6: 6}
        assert n9 + n10 + n11 + n12 + sum(short.values()) == 162
        left = {9: n9, 10: n10, 11: n11, 12: n12}
        pairs, frequent, rare = [], list(vals[:144]), list(vals[144:])
        ln = 9
        for sym in frequent:  # round robin over the lengths that still have codes to give
            while left[ln] == 0:
                ln = 9 + (ln - 8) % 4
            pairs.append((sym, ln))
            left[ln] -= 1
            ln = 9 + (ln - 8) % 4
        pairs += list(zip(rare, [l for l in sorted(short) for _ in range(short[l])]))
        return table(pairs, AC_SYMS)

    dc_l = table(list(zip([11, 10, 9, 8, 7, 6, 0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6, 9, 9, 10, 10, 11, 11])), DC_SYMS)
    dc_c = table(list(zip([11, 10, 9, 8, 7, 6, 5, 0, 1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 9, 10, 10, 11, 11])), DC_SYMS)
    out = (dc_l, ac(s.ANNEX_K_HUFFMAN[1][1], 64, 64, 8, 8), dc_c, ac(s.ANNEX_K_HUFFMAN[3][1], 63, 63, 7, 11))
    for t in out:
        assert {9, 10, 11} <= set(lengths_of(t[0]))
    assert t2_tables(out) <= POOL
    return out


def pool(n):
    """Exactly n second-level tables: the luma AC table has 2n codes of 11 bits (two to a 10-bit prefix; the most
    frequent symbols get them) and the rest 8 bits; every other table stays inside the first level."""
    s = _synth()
    order = list(reversed(s.ANNEX_K_HUFFMAN[1][1]))  # rare symbols first: the short codes
    ac_l = _by_counts(order, {8: 162 - 2 * n, 11: 2 * n}, AC_SYMS)
    dc = _by_counts(DC_SYMS, {4: 12}, DC_SYMS)
    ac_c = _by_counts(AC_SYMS, {8: 162}, AC_SYMS)
    out = (dc, ac_l, dc, ac_c)
    assert [len(t2_prefixes(t)) for t in out] == [0, n, 0, 0]
    return out


def pool_shared():
    """No table's long codes exceed the pool, the four tables together need 25: 10 + 10 + 2 + 3."""
    s = _synth()
    ac = [_by_counts(list(reversed(s.ANNEX_K_HUFFMAN[i][1])), {8: 142, 11: 20}, AC_SYMS) for i in (1, 3)]
    dc_l = _by_counts(DC_SYMS, {4: 8, 11: 4}, DC_SYMS)
    dc_c = _by_counts(DC_SYMS, {4: 6, 11: 6}, DC_SYMS)
    out = (dc_l, ac[0], dc_c, ac[1])
    assert [len(t2_prefixes(t)) for t in out] == [2, 10, 3, 10] and t2_tables(out) == POOL + 1
    return out


FAMILIES = {
    "annexk_reversed": annexk_reversed,
    "flat": flat,
    "complete_allones": complete_allones,
    "all16": all16,
    "unary_dc_long": unary_dc_long,
    "t1_split": t1_split,
    "pool24": lambda: pool(24),
    "pool25": lambda: pool(25),
    "pool_shared": pool_shared,
}
REFUSED = ("pool25", "pool_shared")                         # more second-level tables than a set holds: the host decoder's
TAKEN = tuple(n for n in FAMILIES if n not in REFUSED)      # the device decoder must take and decode these
# families that also run with the Cr component on tables of its own (test_huff_emu.three_table_variant: six tables a set)
THREE_TABLES = ("annexk_reversed", "all16", "t1_split")


def family(name):
    """-> the family's 4-tuple, every table checked."""
    t = FAMILIES[name]()
    assert len(t) == 4
    for i, x in enumerate(t):
        check_table(x, AC_SYMS if i & 1 else DC_SYMS)
    return t


def set_tables(name, three=False):
    """The tables of a frame's set in the order the device decoder builds them (AC tables in use first, then DC), as
    [(is_ac, (BITS, HUFFVAL))]; three: the Cr component on copies of the chroma tables."""
    dc_l, ac_l, dc_c, ac_c = family(name)
    n = 3 if three else 2
    return [(True, t) for t in (ac_l, ac_c, ac_c)[:n]] + [(False, t) for t in (dc_l, dc_c, dc_c)[:n]]


# ---- contents -------------------------------------------------------------------------------------------------------
def full_alphabet_blocks(w, h, hs, vs, seed):
    """Every symbol of the baseline alphabet: |AC| <= 1023, |DC| <= 1000, 40 % zeros, and every third block with
    positions 20..59 zeroed, so that ZRL runs occur."""
    rng = np.random.default_rng(seed)
    n = _synth().geometry(w, h, hs, vs)[3]
    coef = rng.integers(-1023, 1024, size=(n, 64)).astype(np.int16)
    coef[rng.random((n, 64)) < 0.4] = 0
    coef[::3, 20:60] = 0
    coef[:, 0] = rng.integers(-1000, 1001, size=n)
    return coef


def dense_pm1_blocks(w, h, hs, vs, seed):
    """All 64 coefficients of every block +1 or -1 (so a DC difference is 0 or +-2): no EOB anywhere, and under `flat`
    every AC symbol is exactly 9 bits wide -- no block boundary a lane could recognise."""
    rng = np.random.default_rng(seed)
    n = _synth().geometry(w, h, hs, vs)[3]
    coef = (rng.integers(0, 2, size=(n, 64)) * 2 - 1).astype(np.int16)
    return coef


def contents(w, h, hs, vs, seed=0):
    """-> {"synth": ..., "full": ...}: (coef, qtabs) of the two kinds of content every family is coded with."""
    s = _synth()
    c, q = s.synth_blocks(w, h, hs, vs, 70 + seed)
    return {"synth": (c, q), "full": (full_alphabet_blocks(w, h, hs, vs, 7 + seed), s.annex_k_qtabs(75))}


# ---- streams the writer cannot make ---------------------------------------------------------------------------------
def hand_tables():
    """Annex K's tables with symbols in them that no writer emits: in the luma AC table the run-only symbols 0x10..0xE0
    (the reference reads them as `run` zeros and no coefficient) stand where 0x1A..0xEA stood (runs with a size-10
    coefficient, which these streams do not use: the table keeps K.5's shape and its 162 symbols, all the reference's
    tables hold); in the chroma AC table 0x0B, a size-11 coefficient, stands for 0xFA; the luma DC table also holds
    size 12, on a 10-bit code K.3 leaves free."""
    s = _synth()
    dc = (list(s.ANNEX_K_HUFFMAN[0][0]), list(s.ANNEX_K_HUFFMAN[0][1]) + [12])
    dc[0][9] += 1
    ac_l = (list(s.ANNEX_K_HUFFMAN[1][0]), [v & 0xf0 if v & 15 == 10 and 1 <= v >> 4 <= 14 else v for v in s.ANNEX_K_HUFFMAN[1][1]])
    ac_c = (list(s.ANNEX_K_HUFFMAN[3][0]), [0x0b if v == 0xfa else v for v in s.ANNEX_K_HUFFMAN[3][1]])
    for t in (dc, ac_l, ac_c):
        check_table(t)
    assert {r << 4 for r in range(1, 15)} <= set(ac_l[1]) and len(ac_l[1]) == 162 and 0x0b in ac_c[1] and 12 in dc[1]
    return dc, ac_l, s.ANNEX_K_HUFFMAN[2], ac_c


class BitWriter:
    """MSB-first bits -> bytes with JPEG byte stuffing; the last byte is padded with ones."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xff
            self.out.append(b)
            if b == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    """-> (size, bits) of a coefficient value (T.81 F.1.2.1)."""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


class Enc:
    """Symbols of one table -> bits."""

    def __init__(self, t):
        self.code = {sym: (ln, code) for sym, (ln, code) in zip(t[1], codes_of(t[0]))}

    def sym(self, bw, s):
        ln, code = self.code[s]
        bw.put(code, ln)


def _put_block(bw, dc, ac, diff, zz):
    """A block the ordinary way: DC difference, then run/size symbols, ZRL, EOB.  zz: 63 AC values in zig-zag order."""
    size, bits = _magnitude(diff)
    dc.sym(bw, size)
    bw.put(bits, size)
    run = 0
    for v in zz:
        if v == 0:
            run += 1
            continue
        while run > 15:
            ac.sym(bw, 0xf0)
            run -= 16
        size, bits = _magnitude(int(v))
        ac.sym(bw, (run << 4) | size)
        bw.put(bits, size)
        run = 0
    if run:
        ac.sym(bw, 0x00)


def hand_streams(w=64, h=48):
    """-> {name: (jpeg bytes, expected blocks or None)}: 4:4:4 streams of w x h (144 blocks, some 3 KB of scan: more
    than 16 chunks of 128 bytes) coded by the bit writer above with hand_tables(); block 3 (the luma block of the second
    MCU; for ac_size_11 block 4, its Cb block) is written symbol by symbol.  Accepted cases come with the blocks they must decode to; for the others (None)
    a decoder's verdict is all there is.
      run_only_mid   0x01 at k=1, run-only 0x30 (three zeros, no coefficient), 0x01 at k=5, EOB
      zrl_at_47      0x01 at k=1..46, ZRL at k=47 (k -> 63), 0x01 at k=63: the block ends without EOB
      run_to_63      0x01 at k=1..59, then 0x31 at k=60: k + run = 63, the block ends without EOB
      zrl_at_48      0x01 at k=1..47, ZRL at k=48: k + 16 = 64 leaves the block
      run_to_64      0x01 at k=1..60, then 0x31 at k=61: k + run = 64 leaves the block
      dc_size_12     the DC symbol 12 (in the table, no decoder takes it)
      ac_size_11     the AC symbol 0x0B at k=1"""
    s = _synth()
    tabs = hand_tables()
    rng = np.random.default_rng(12)
    n = s.geometry(w, h, 1, 1)[3]
    zz_of = s.ZIGZAG
    base = np.zeros((n, 64), np.int16)
    # padding blocks: dense small values, so that the scan is long enough for many chunks
    base[:, zz_of] = rng.integers(-3, 4, size=(n, 64))
    base[:, 0] = rng.integers(-40, 41, size=n)
    head = s.encode_jpeg(base, w, h, 1, 1, s.annex_k_qtabs(90), huffman=tabs)
    sos = head.index(b"\xff\xda")
    head = head[:sos + 2 + ((head[sos + 2] << 8) | head[sos + 3])]  # everything up to the scan's first byte
    dcs, acs = (Enc(tabs[0]), Enc(tabs[2])), (Enc(tabs[1]), Enc(tabs[3]))

    def script(name, bw, ac, blk):
        """writes block `special`'s AC part; fills blk (zig-zag order) with what it must decode to, or returns False"""
        def coefs(k0, k1):  # 0x01 symbols for positions k0..k1-1, alternating signs
            for k in range(k0, k1):
                v = 1 if k & 1 else -1
                ac.sym(bw, 0x01)
                bw.put(1 if v > 0 else 0, 1)
                blk[k] = v
        if name == "run_only_mid":
            coefs(1, 2)
            ac.sym(bw, 0x30)
            coefs(5, 6)
            ac.sym(bw, 0x00)
        elif name == "zrl_at_47":
            coefs(1, 47)
            ac.sym(bw, 0xf0)
            coefs(63, 64)
        elif name == "run_to_63":
            coefs(1, 60)
            ac.sym(bw, 0x31)
            bw.put(1, 1)
            blk[63] = 1
        elif name == "zrl_at_48":
            coefs(1, 48)
            ac.sym(bw, 0xf0)
            ac.sym(bw, 0x00)
            return False
        elif name == "run_to_64":
            coefs(1, 61)
            ac.sym(bw, 0x31)
            bw.put(1, 1)
            return False
        elif name == "ac_size_11":
            ac.sym(bw, 0x0b)
            bw.put(0x5a5, 11)
            ac.sym(bw, 0x00)
            return False
        else:
            raise KeyError(name)
        return True

    out = {}
    for name in ("run_only_mid", "zrl_at_47", "run_to_63", "zrl_at_48", "run_to_64", "dc_size_12", "ac_size_11"):
        bw = BitWriter()
        special = 4 if name == "ac_size_11" else 3
        want = base.copy()
        pred = [0, 0, 0]
        ok = True
        for b in range(n):
            c = b % 3
            dc, ac = dcs[min(c, 1)], acs[min(c, 1)]
            if b != special:
                _put_block(bw, dc, ac, int(base[b, 0]) - pred[c], base[b, zz_of][1:])
                pred[c] = int(base[b, 0])
                continue
            if name == "dc_size_12":
                dc.sym(bw, 12)
                bw.put(0xa5a, 12)
                ac.sym(bw, 0x00)
                ok = False
                continue
            size, bits = _magnitude(int(base[b, 0]) - pred[c])
            dc.sym(bw, size)
            bw.put(bits, size)
            pred[c] = int(base[b, 0])
            blk = np.zeros(64, np.int16)
            blk[0] = base[b, 0]
            ok = script(name, bw, ac, blk)
            want[b, zz_of] = blk
        out[name] = (head + bw.finish() + b"\xff\xd9", want if ok else None)
    return out


HAND_ACCEPTED = ("run_only_mid", "zrl_at_47", "run_to_63")
HAND_REJECTED = ("zrl_at_48", "run_to_64", "dc_size_12", "ac_size_11")


# ---- the genuine reference, in a child process (it calls exit(1) on what it rejects) --------------------------------
def ref_dump_main(paths):
    """For every file: the reference's decodeHuffman() coefficients -> <file>.ref.npy.  A file the reference rejects
    ends the process with its exit(1); the files before it are done."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.pyoracle import Ref
    ref = Ref()
    for p in paths:
        np.save(p + ".ref.npy", ref.decode_file(p)[1])
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--ref-dump":
        sys.exit(ref_dump_main(sys.argv[2:]))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in FAMILIES:
        t = family(name)
        print(f"{name}: second-level tables {[len(t2_prefixes(x)) for x in t]}, Kraft/65536 {[kraft(x[0]) for x in t]}, "
              f"longest code {[max(lengths_of(x[0])) for x in t]}")
