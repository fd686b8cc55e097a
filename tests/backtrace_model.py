"""Executable statement of the light backtrace's two walks (csrc/wave_viterbi.hip, backtrace_light_body) over a
packed back-pointer table of one channel, in plain Python integers.

    walk_samples   the per-sample rule (HS_BT_EVENTS = 0): one step per sample, with the wave-uniform choice
                   between the fast tile bodies and the one with per-lane time marks
    walk_events    the event walk (HS_BT_EVENTS = 1): row masks, jumps over rings and silence, ramps, and the
                   expansion of the ramps where x is stored

Both return (x, bs, nflag): the decoded ids (-1 where the kernel stores nothing), the id every segment but the
last finds at its successor's first sample, and the flagged decisions met inside the owned segments.  They must
agree on ANY table, not only on tables a Viterbi sweep writes (tests/test_backtrace_model_cpu.py).

psi is an integer array [PW][T]: entry e (0 = silent, a + 1 = ring a) of sample t sits in word e // EPW at bit
(e % EPW) * EB; its low EB - 1 bits name the predecessor (0 silent, p = last state of ring p - 1), the top bit is
the near-tie flag.  State ids are 1-based: 1 silent, 1 + a L + k the k-th state of ring a.
"""
import numpy as np


def packing(N):
    """(EB, EPW, PW) of wave_common.h: bits per entry with the flag, entries per word, words per sample"""
    b = 1
    while (1 << b) < N + 1:
        b += 1
    EB = b + 1
    EPW = 32 // EB
    return EB, EPW, (N + 1 + EPW - 1) // EPW


def tile_samples(N):
    PW = packing(N)[2]
    return 64 if PW == 1 else (32 if PW <= 3 else 16)


def segments_per_group(N):
    return 32 if packing(N)[2] == 1 else 64


def seg_geometry(L):
    """make_geometry's backtrace segments: length Bb and walk-in Hb (csrc/wave_engine.hip)"""
    Bb, Hb = 512, 128
    while Hb < 2 * L + 64:
        Hb += 64
    return max(Bb, 2 * Hb), Hb


def pack_table(N, pred, flag):
    """pred, flag: [N + 1][T] predecessor fields and flag bits -> psi[PW][T]"""
    EB, EPW, PW = packing(N)
    T = pred.shape[1]
    psi = np.zeros((PW, T), dtype=np.int64)
    for e in range(N + 1):
        psi[e // EPW] |= (pred[e].astype(np.int64) | (flag[e].astype(np.int64) << (EB - 1))) << ((e % EPW) * EB)
    return psi


class _Lane:
    """what a lane derives from its segment number (the top of backtrace_light_body)"""

    def __init__(self, sg, nseg, T, Bb, Hb, N, L, fs):
        EB, EPW, _ = packing(N)
        self.active = sg < nseg
        s_lo = sg * Bb
        s_hi = min(s_lo + Bb, T) if self.active else s_lo
        te = min(s_hi + Hb, T)
        self.s_lo = s_lo
        self.te_rel = te - s_lo if self.active else 0
        self.hi_rel = s_hi - s_lo
        self.t1 = 0 if s_lo >= 1 else 1
        self.t2 = 2 * self.t1
        self.id, self.rem, self.wi, self.sh = 1, 0, 0, 0
        if self.active and te == T and fs > 0:      # bt_start: the walk that starts at T starts from the final state
            a0, k0 = (fs - 1) // L, (fs - 1) % L + 1
            e0 = a0 + 1
            self.id, self.rem, self.wi, self.sh = fs + 1, k0 - 1, e0 // EPW, (e0 % EPW) * EB
        self.bs = 0
        self.u = self.te_rel - 1                    # event walk: next sample to decide


def _stage(psi, T, lanes, u0, TS):
    """the tile in LDS: tile[w][r][c] = psi[w][s_lo(r) + u0 + c], zeros for rows that do not exist and past T"""
    PW = psi.shape[0]
    tile = np.zeros((PW, len(lanes), TS), dtype=np.int64)
    for r, ln in enumerate(lanes):
        if not ln.active:
            continue
        t0 = ln.s_lo + u0
        n = max(0, min(TS, T - t0))
        if n:
            tile[:, r, :n] = psi[:, t0:t0 + n]
    return tile


def _fast(lanes, u0, TS, Bb):
    u1, own = u0 + TS, u0 < Bb
    return all(u0 >= ln.t1 and u1 <= ln.te_rel and
               ((u1 <= ln.hi_rel and u0 >= ln.t2) if own else (u0 > ln.hi_rel)) for ln in lanes)


def _junction(N, L, ent):
    EB, EPW, _ = packing(N)
    pj = ent & ((1 << (EB - 1)) - 1)
    return 1 + pj * L, (L - 1 if pj else 0), pj // EPW, (pj % EPW) * EB, (ent >> (EB - 1)) & 1


def _run(psi, T, N, L, Bb, Hb, fs, tile_body):
    TS, SPW = tile_samples(N), segments_per_group(N)
    nseg = (T + Bb - 1) // Bb
    x = np.full(T, -1, dtype=np.int64)
    bs = np.zeros(max(nseg - 1, 0), dtype=np.int64)
    nflag = 0
    for sg0 in range(0, nseg, SPW):
        lanes = [_Lane(sg0 + r, nseg, T, Bb, Hb, N, L, fs) for r in range(SPW)]
        for q in range((Bb + Hb) // TS - 1, -1, -1):
            u0 = TS * q
            tile = _stage(psi, T, lanes, u0, TS)
            own, fast = u0 < Bb, _fast(lanes, u0, TS, Bb)
            out = np.ones((SPW, TS), dtype=np.int64)        # what the store phase sees for this tile
            for r, ln in enumerate(lanes):
                nflag += tile_body(ln, tile[:, r, :], u0, TS, N, L, fast, own, out[r])
            if own:
                for r, ln in enumerate(lanes):
                    if ln.active:
                        t0 = ln.s_lo + u0
                        n = max(0, min(TS, T - t0))
                        x[t0:t0 + n] = out[r, :n]
        for r, ln in enumerate(lanes):
            if sg0 + r < nseg - 1:
                bs[sg0 + r] = ln.bs
    return x, bs, nflag


def _samples_body(ln, row, u0, TS, N, L, fast, own, out):
    nflag = 0
    for i in range(TS - 1, -1, -1):
        u = u0 + i
        interior = ln.rem > 0
        out[i] = ln.id
        jid, jrem, jwi, jsh, flag = _junction(N, L, int(row[ln.wi, i]) >> ln.sh)
        if fast:
            if own and not interior:
                nflag += flag
            step = True
        else:
            live = u < ln.te_rel
            step = live and u >= ln.t1
            if live and u == ln.hi_rel:
                ln.bs = ln.id
            if step and not interior and u < ln.hi_rel and u >= ln.t2:
                nflag += flag
        if step:
            if interior:
                ln.id, ln.rem = ln.id - 1, ln.rem - 1
            else:
                ln.id, ln.rem, ln.wi, ln.sh = jid, jrem, jwi, jsh
    return nflag


def _low(p):
    return (2 << p) - 1


def _events_body(ln, row, u0, TS, N, L, fast, own, out):
    EB = packing(N)[0]
    pjm = (1 << (EB - 1)) - 1
    # masks of the row: entry 0 sits in word 0 at bit 0
    pm = sum(1 << c for c in range(TS) if int(row[0, c]) & pjm)
    fm = sum(1 << c for c in range(TS) if (int(row[0, c]) >> (EB - 1)) & 1) if own else 0
    nflag = 0
    ramps = []
    while ln.u >= u0:
        u = ln.u
        p = u - u0
        assert p < TS
        if ln.id == 1:
            below = pm & _low(p)
            j = below.bit_length() - 1 if below else -1
            if not fast and u0 + j < ln.t1:
                j = -1
            lo = max(j, 0)
            if own or not fast:
                a, b = lo, p
                if not fast:
                    a, b = max(a, ln.t2 - u0), min(b, ln.hi_rel - 1 - u0)
                if a <= b:
                    nflag += bin(fm & _low(b) & ~_low(a - 1) if a else fm & _low(b)).count("1")
            if not fast and lo <= ln.hi_rel - u0 <= p:
                ln.bs = 1
            if j < 0:
                ln.u = u0 - 1
                break
            pj = int(row[0, j]) & pjm
            ln.id, ln.rem, ln.wi, ln.sh = _junction(N, L, pj)[:4]
            ln.u = u0 + j - 1
        else:
            s = min(ln.rem, p + 1)
            junc = s <= p
            n = s + (1 if junc else 0)
            ramps.append((p - n + 1, p, ln.id))
            if not fast:
                d = u - ln.hi_rel
                if 0 <= d < n:
                    ln.bs = ln.id - d
            if junc:
                uj = u - s
                if fast or uj >= ln.t1:
                    jid, jrem, jwi, jsh, flag = _junction(N, L, int(row[ln.wi, uj - u0]) >> ln.sh)
                    if (own if fast else (uj < ln.hi_rel and uj >= ln.t2)):
                        nflag += flag
                    ln.id, ln.rem, ln.wi, ln.sh = jid, jrem, jwi, jsh
            else:
                ln.id, ln.rem = ln.id - s, ln.rem - s
            ln.u = u - n
    assert len(ramps) <= TS // 8 + 2, (len(ramps), TS, L)
    for f, l, idl in ramps:                                  # the store phase
        assert 0 <= f <= l < 64 and idl < (1 << 20)
        for c in range(f, l + 1):
            out[c] = idl - l + c
    return nflag


def walk_samples(psi, T, N, L, Bb, Hb, fs=0):
    return _run(psi, T, N, L, Bb, Hb, fs, _samples_body)


def walk_events(psi, T, N, L, Bb, Hb, fs=0):
    return _run(psi, T, N, L, Bb, Hb, fs, _events_body)


def walk_plain(psi, T, N, L, fs=0):
    """the path of the whole table walked in one piece from the final state (what the segments' walks reproduce
    once they have merged): x only"""
    EB, EPW, _ = packing(N)
    x = np.zeros(T, dtype=np.int64)
    idv, rem, wi, sh = 1, 0, 0, 0
    if fs > 0:
        a0, k0 = (fs - 1) // L, (fs - 1) % L + 1
        idv, rem, wi, sh = fs + 1, k0 - 1, (a0 + 1) // EPW, ((a0 + 1) % EPW) * EB
    for t in range(T - 1, -1, -1):
        x[t] = idv
        if t == 0:
            break
        if rem > 0:
            idv, rem = idv - 1, rem - 1
        else:
            idv, rem, wi, sh = _junction(N, L, int(psi[wi, t]) >> sh)[:4]
    return x
