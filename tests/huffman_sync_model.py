"""A symbol-level model of the parallel Huffman decoder's convergence
(k_huff_image, csrc/ldt_huffman.hip image_decode), in plain Python (a test
helper: tests import it, nothing else does).

``model(jpeg, S)`` takes a baseline JPEG and the subsequence length S the
planner gave it and plays the scheme per restart segment:

* the state machine (p, b, k) over the destuffed bits -- bit position, block
  within the MCU, coefficient index -- which is jdhuff.c's block loop: DC
  symbol (k: 0 -> 1), AC symbols (k += run + 1, ZRL 16, EOB ends the block).
  An unknown code skips 16 bits and gives symbol 0 (ldt_types.hpp), bits past
  the segment read as zero;
* ranges [j*S, min((j+1)*S, seg_bits)), one slot each (at least one per
  segment);
* phase 1: slot j decodes from (max(j*S - warm, 0), 0, 0) up to j*S (its
  entry) and on to the first symbol boundary >= its range end (its exit);
* rounds: in slot order every slot keeps its trajectory C if its predecessor's
  chosen exit equals C's entry, else adopts its previous trajectory M (the
  memo) if the exit equals M's entry, else is needy: C becomes M and the slot
  is decoded again from the predecessor's chosen exit. The rounds end when no
  slot is needy or no exit changed, and are counted as the kernel counts them
  (every iteration, the last one included: a stream that needs no re-decode
  has 1 round).

It asserts by itself that the final entries are those of a serial walk.

Limits. The kernel's checkpoint merges end a re-decode early without changing
any state, so they are left out. Its count-mode steps consume several AC
symbols of one block per lookup, so an exit may lie a few symbols further
than here: the model is exact only where every step is one symbol, which
``single_symbol_steps`` reports (no block of the file holds an AC symbol other
than EOB).
"""
from collections import namedtuple

import numpy as np

import jpeg_recode as jr

PAD_BITS = 64  # zero bits after a segment (the kernel's kSegPad bytes)

# per segment: needy[r] = needy slots of round r (the last round's 0 included)
SegResult = namedtuple("SegResult", "bits slots rounds adoptions needy")
# per image: rounds = the kernel's loop iterations (max over segments), needy
# and adoptions summed over rounds and segments, wide = rounds with more than
# 64 needy slots in the image (a work list that spans waves)
Result = namedtuple("Result", "S slots rounds adoptions needy wide segments")


def _luts(jpeg: bytes):
    """{(tc, th): (total bits[65536], k advance[65536])} by the next 16 bits,
    as ldt_types.hpp huff_entry defines them."""
    out = {}
    for tc, th, counts, symbols in jr.dht_tables(jpeg):
        tot = np.full(65536, 16, np.int32)
        adv = np.full(65536, 1 if tc == 0 else 64, np.int32)
        for sym, length, code in jr.canonical(counts, symbols):
            lo, hi = code << (16 - length), (code + 1) << (16 - length)
            if tc == 0:
                s, a = sym, 1
            else:
                s, r = sym & 15, sym >> 4
                a = r + 1 if s else (16 if r == 15 else 64)
            tot[lo:hi] = length + s
            adv[lo:hi] = a
        out[tc, th] = (tot, adv)
    return out


class Stream:
    """One restart segment: step tables per block of the MCU."""

    def __init__(self, data: bytes, frame, luts):
        self.bits = 8 * len(data)
        n = self.bits + 32
        b = np.unpackbits(np.frombuffer(data + b"\x00" * (PAD_BITS // 8), np.uint8)).astype(np.int32)
        w = np.zeros(n, np.int32)
        for i in range(16):
            w = (w << 1) | b[i:i + n]
        self.bpm = len(frame.blocks)
        per_tab = {key: (tot[w].tolist(), adv[w].tolist()) for key, (tot, adv) in luts.items()}
        self.dc, self.ac = [], []
        for ci in frame.blocks:
            td, ta = frame.sel[frame.comps[ci][0]]
            self.dc.append(per_tab[0, td])
            self.ac.append(per_tab[1, ta])

    def step(self, p, b, k):
        tot, adv = (self.dc if k == 0 else self.ac)[b]
        k += adv[p]
        p += tot[p]
        if k >= 64:
            b, k = (b + 1 if b + 1 < self.bpm else 0), 0
        return p, b, k

    def run(self, p, b, k, stop):
        """The state at the first symbol boundary >= stop."""
        dc, ac, bpm = self.dc, self.ac, self.bpm
        while p < stop:
            tot, adv = (dc if k == 0 else ac)[b]
            k += adv[p]
            p += tot[p]
            if k >= 64:
                b, k = (b + 1 if b + 1 < bpm else 0), 0
        return p, b, k


def _segment(st: Stream, S: int, warm: int, memo: bool) -> SegResult:
    n = max(1, -(-st.bits // S))
    stops = [min((j + 1) * S, st.bits) for j in range(n)]
    en, ex = [], []
    for j in range(n):
        e = st.run(max(j * S - warm, 0), 0, 0, j * S)
        en.append(e)
        ex.append(st.run(*e, stops[j]))
    m_en, m_ex = [None] * n, [None] * n
    rounds = adoptions = 0
    needy = []
    while True:
        assert rounds <= n, "more rounds than slots"
        rounds += 1
        work = []
        prev = ex[0]  # the predecessor's chosen exit; slot 0 keeps C
        for j in range(1, n):
            if prev == en[j]:
                prev = ex[j]
            elif memo and prev == m_en[j]:
                en[j], m_en[j] = m_en[j], en[j]
                ex[j], m_ex[j] = m_ex[j], ex[j]
                adoptions += 1
                prev = ex[j]
            else:
                m_en[j], m_ex[j] = en[j], ex[j]
                en[j] = prev
                work.append(j)
                prev = ex[j]  # a needy slot's exit is still its old one
        needy.append(len(work))
        if not work:
            break
        changed = False
        for j in work:
            x = st.run(*en[j], stops[j])
            changed = changed or x != ex[j]
            ex[j] = x
        if not changed:
            break
    # the final entries are a serial walk's
    s = (0, 0, 0)
    for j in range(n):
        assert en[j] == s and (j == 0 or ex[j - 1] == s), "slot %d: entry %r, serial %r" % (j, en[j], s)
        s = st.run(*s, stops[j])
    assert ex[n - 1] == s
    return SegResult(st.bits, n, rounds, adoptions, needy)


def streams(jpeg: bytes):
    """The Stream of each restart segment."""
    segs, ecs = jr.parse(jpeg)
    frame, luts = jr._frame(segs), _luts(jpeg)
    return [Stream(d, frame, luts) for d in jr._intervals(ecs)]


def slot_counts(jpeg: bytes, S: int):
    """Slots of each restart segment, as the kernel cuts them."""
    return [max(1, -(-8 * len(d) // S)) for d in jr._intervals(jr.parse(jpeg)[1])]


def model(jpeg: bytes, S: int, warm_pct: int = 0, memo: bool = True) -> Result:
    """The rounds of `jpeg` under subsequences of S bits (warm_pct as
    LDT_OPT_SYNC_WARM; memo=False: no slot ever adopts its memo)."""
    segs = [_segment(st, S, (S * warm_pct) // 100, memo) for st in streams(jpeg)]
    rounds = max(s.rounds for s in segs)
    per_round = [sum(s.needy[r] for s in segs if r < len(s.needy)) for r in range(rounds)]
    return Result(S, sum(s.slots for s in segs), rounds, sum(s.adoptions for s in segs), sum(per_round),
                  sum(1 for x in per_round if x > 64), tuple(segs))


def never_merges(jpeg: bytes, S: int):
    """Per restart segment, [never_merges(j) for each slot j]: the guess
    trajectory of slot j, from (j*S, 0, 0), shares no state with the true
    trajectory up to the segment's end. (Slot 0's guess is the truth: False.)"""
    out = []
    for st in streams(jpeg):
        true = set()
        s = (0, 0, 0)
        while s[0] < st.bits:
            true.add(s)
            s = st.step(*s)
        fate = {}  # state -> True: no trajectory through it meets the truth
        res = []
        for j in range(max(1, -(-st.bits // S))):
            s, path = (j * S, 0, 0), []
            while True:
                if s in true:
                    r = False
                elif s in fate:
                    r = fate[s]
                elif s[0] >= st.bits:
                    r = True
                else:
                    path.append(s)
                    s = st.step(*s)
                    continue
                break
            for q in path:
                fate[q] = r
            res.append(r)
        out.append(res)
    return out


def single_symbol_steps(jpeg: bytes) -> bool:
    """No block holds an AC symbol other than EOB: every count-mode step of
    the true trajectory is one symbol, and the model is exact."""
    return all(sym == 0 for syms in jr.scan_symbols(jpeg) for _, tc, sym, _ in syms if tc == 1)
