"""Plain Python / NumPy restatement of docs/JPEG.md §12: Huffman decoding of a baseline scan by self-synchronising subsequences, the
way csrc/ss_jpeg.hip's k_jpeg_huff and k_jpeg_dc do it.  The specification in executable form; not a test module.

    raw, segs = cut(data)                       the host's pass: unstuffed scan bytes, [(byte offset, byte length, first block, blocks)]
    coef, rounds, status = decode(data, W=32)   dense int16 blocks in ss_jpeg_coefficients' layout, the rounds each tile took,
                                                None or the cause the device reports (then every block is empty)
    st = stream(data, W); finish(st)            the same in two steps; entry_count(st): (entries of the stream, the capacity derived
                                                from the scan's length)

Header refusals and "bad restart marker" raise jpeg_ref.Refused, as the host's pass refuses them before any launch.
"""
import numpy as np

from tests.jpeg_ref import Refused, ZIGZAG, parse

LANES = 1024                                     # subsequences of a tile
CAUSES = {1: "Huffman code that does not exist", 2: "bad DC category", 3: "coefficient index beyond 63", 4: "data ends before the last MCU",
          5: "bad restart marker", 6: "more entries than the scan's length allows"}


def _geometry(info):
    comps = info["comps"]
    hv = 1 if len(comps) == 1 else comps[0][1] * comps[0][2]
    bpm = 1 if len(comps) == 1 else hv + 2
    return hv, bpm, info["mcux"] * info["mcuy"]


def cut(data, info=None):
    """One pass over the scan: drop the 00 after every FF, cut at the RSTn markers (FF fill bytes before a marker tolerated), stop at
    the first other marker, pad every segment with zeros to 4 bytes."""
    d = bytes(data)
    info = info or parse(d)
    hv, bpm, nm = _geometry(info)
    ri = info["ri"] or nm
    nseg = -(-nm // ri)
    n, p = len(d), info["scan"]
    out, segs = bytearray(), []
    for sg in range(nseg):
        start = len(out)
        while True:
            q = d.find(b"\xff", p)
            q = n if q < 0 else q
            out += d[p:q]
            p = q
            if p + 1 < n and d[p + 1] == 0:
                out.append(0xFF)
                p += 2
                continue
            break
        ln = len(out) - start
        out += b"\0" * (-len(out) % 4)
        m0 = sg * ri
        segs.append((start, ln, m0 * bpm, min(ri, nm - m0) * bpm))
        if sg + 1 < nseg:
            q = p
            while q < n and d[q] == 0xFF:
                q += 1
            if q >= n or q == p or d[q] != 0xD0 + (sg & 7):
                raise Refused("bad restart marker")
            p = q + 1
    return bytes(out), segs


def _lut(table):
    """16 leading bits -> (length << 8) | symbol, 0: no such code (the kernel's two levels give the same answer)."""
    lut = np.zeros(65536, np.int32)
    for (ln, code), sym in table.items():
        lut[code << (16 - ln):(code + 1) << (16 - ln)] = (ln << 8) | sym
    return lut.tolist()


class _Sink:
    def __init__(self, tab, ent, cap):
        self.tab, self.ent, self.cap = tab, ent, cap
        self.e = self.blk = self.bend = self.err = 0
        self.last_seg = False


def _decode(luts, w, bits, end, hv, bpm, state, maxbegin, sink=None):
    """From `state` every symbol that starts before bit `end`, beginning at most `maxbegin` blocks.  Total: a code that does not exist
    consumes one bit, a DC category above 15 keeps its low four bits, a run beyond index 63 closes the block.  Returns the exit
    state, blocks begun, entries, entries before the last block begun."""
    p, bi, k = state
    nb = ne = nel = 0
    nw = len(w) - 2                                               # (two zero words follow: reads beyond supply zero bits)
    while p < end:
        if k == 0 and nb >= maxbegin:
            break
        i, sh = p >> 5, p & 31
        win = ((((w[i] << 32) | w[i + 1]) >> (32 - sh)) & 0xFFFFFFFF) if i < nw else 0
        comp = 0 if bi < hv else bi - hv + 1
        f = luts[2 * comp + (1 if k else 0)][win >> 16]
        if not f:
            if sink is not None and not sink.err:
                sink.err = 4 if bits - p < 16 else 1
            p += 1
            continue
        ln, sym = f >> 8, f & 255
        close = False
        if k == 0:
            s = sym
            if s > 15:
                if sink is not None and not sink.err:
                    sink.err = 2
                s &= 15
            v = 0
            if s:
                v = ((win << ln) & 0xFFFFFFFF) >> (32 - s)
                if v < (1 << (s - 1)):
                    v = v - (1 << s) + 1
            nel = ne
            if sink is not None:
                assert sink.blk < sink.bend                     # `maxbegin` keeps every table store inside the lane's segment, whatever the bits say
                if sink.e < sink.cap:
                    sink.tab[sink.blk] = sink.e
                    sink.ent[sink.e] = v & 0xFFFF
                elif not sink.err:
                    sink.err = 6
                sink.blk += 1
                sink.e += 1
            nb += 1
            ne += 1
            p += ln + s
            k = 1
        else:
            r, s = sym >> 4, sym & 15
            if not s:
                p += ln
                if r == 15:
                    k += 16
                    close = k > 63
                else:
                    close = True
            else:
                k += r
                if k > 63:
                    if sink is not None and not sink.err:
                        sink.err = 3
                    p += ln
                    close = True
                else:
                    v = ((win << ln) & 0xFFFFFFFF) >> (32 - s)
                    if v < (1 << (s - 1)):
                        v = v - (1 << s) + 1
                    if sink is not None:
                        if sink.e < sink.cap:
                            sink.ent[sink.e] = (int(ZIGZAG[k]) << 16) | (v & 0xFFFF)
                        elif not sink.err:
                            sink.err = 6
                        sink.e += 1
                    ne += 1
                    p += ln + s
                    k += 1
                    close = k == 64
        if close:
            k = 0
            bi = 0 if bi + 1 == bpm else bi + 1
            if sink is not None and sink.blk == sink.bend:      # the segment's last block: what is left over?
                if p > bits:
                    sink.err = sink.err or 4
                elif not sink.last_seg and bits - p >= 8:
                    sink.err = sink.err or 5
                break
    return (p, bi, k), nb, ne, nel


def stream(data, W=32, lanes_per_tile=LANES, errors=None):
    """The device stream of one image: (info, block table [blocks + 1], entries, rounds per tile, status word or None, capacity).
    The status word is `(lane + 1) << 3 | cause` of the smallest lane that reports; `errors` (a list) receives every lane's word."""
    d = bytes(data)
    info = parse(d)
    raw, segs = cut(d, info)
    hv, bpm, nm = _geometry(info)
    blocks = nm * bpm
    luts = []
    for (td, ta) in info["sel"]:
        luts += [_lut(info["dc"][td]), _lut(info["ac"][ta])]
    cap = blocks + 4 * sum(s[1] for s in segs)
    tab, ent = [0] * (blocks + 1), [0] * cap
    # lanes: (segment, index in the segment)
    lane_seg, lane0 = [], []
    for si, (off, ln, blk0, nblk) in enumerate(segs):
        lane0.append(len(lane_seg))
        lane_seg += [si] * max(1, -(-ln // (4 * W)))
    lanes = len(lane_seg)
    words = []
    for (off, ln, _, _) in segs:
        words.append(np.frombuffer(raw[off:off + (ln + 3) // 4 * 4], ">u4").tolist() + [0, 0])
    rounds, status = [], None
    carry_state, carry_blk, carry_ent = (0, 0, 0), 0, 0
    for tile0 in range(0, lanes, lanes_per_tile):
        nl = min(lanes_per_tile, lanes - tile0)
        L = []
        for t in range(nl):
            g = tile0 + t
            si = lane_seg[g]
            off, ln, blk0, nblk = segs[si]
            j = g - lane0[si]
            L.append(dict(si=si, j=j, w=words[si], bits=8 * ln, end=min((j + 1) * 32 * W, 8 * ln), blk0=blk0, nblk=nblk,
                          last=(g + 1 == lanes or lane_seg[g + 1] != si), exact=(j == 0 or t == 0),
                          entry=(carry_state if (j != 0 and t == 0) else (j * 32 * W, 0, 0))))
        # round 0 from the guess, then from the left neighbour's exit state while it differs
        res = [_decode(luts, l["w"], l["bits"], l["end"], hv, bpm, l["entry"], 1 << 31) for l in L]
        r = 1
        for _ in range(1, nl):
            ex = [x[0] for x in res]
            redo = [t for t in range(nl) if not L[t]["exact"] and ex[t - 1] != L[t]["entry"]]
            if not redo:
                break
            r += 1
            for t in redo:
                L[t]["entry"] = ex[t - 1]
                res[t] = _decode(luts, L[t]["w"], L[t]["bits"], L[t]["end"], hv, bpm, L[t]["entry"], 1 << 31)
        rounds.append(r)
        # blocks begun in the lane's segment before it; the counts of a lane in which the segment's blocks end
        bex = np.concatenate([[0], np.cumsum([x[1] for x in res])]).tolist()
        counts = []
        for t, l in enumerate(L):
            first = max(lane0[l["si"]] - tile0, 0)
            b0 = bex[t] - bex[first] + (carry_blk if lane0[l["si"]] < tile0 else 0)
            l["b0"] = b0
            mb = l["maxbegin"] = -1 if b0 > l["nblk"] else l["nblk"] - b0
            _, nb, ne, nel = res[t]
            if mb < 0:
                ne = 0
            elif nb > mb:
                if nb == mb + 1:
                    ne = nel
                else:
                    ne = _decode(luts, l["w"], l["bits"], l["end"], hv, bpm, l["entry"], mb)[2]
            counts.append(ne)
        eex = np.concatenate([[0], np.cumsum(counts)]).tolist()
        # the storing pass
        for t, l in enumerate(L):
            if l["maxbegin"] < 0:
                continue
            s = _Sink(tab, ent, cap)
            s.e, s.blk, s.bend, s.last_seg = carry_ent + eex[t], l["blk0"] + l["b0"], l["blk0"] + l["nblk"], l["si"] + 1 == len(segs)
            (p, bi, k), _, _, _ = _decode(luts, l["w"], l["bits"], l["end"], hv, bpm, l["entry"], l["maxbegin"], s)
            if l["last"] and not s.err and not (s.blk == s.bend and k == 0):
                s.err = 4
            if s.err:
                key = ((tile0 + t + 1) << 3) | s.err
                if errors is not None:
                    errors.append(key)
                status = key if status is None else min(status, key)
        carry_state, carry_blk, carry_ent = res[-1][0], L[-1]["b0"] + res[-1][1], carry_ent + eex[-1]
    tab[blocks] = carry_ent
    return info, tab, ent, rounds, status, cap


def decode(data, W=32, lanes_per_tile=LANES):
    return finish(stream(data, W, lanes_per_tile))


def finish(st):
    """k_jpeg_dc and the expansion of a stream() into dense blocks: (coefficients, rounds, None or the cause)."""
    info, tab, ent, rounds, status, cap = st
    ent = list(ent)
    comps = info["comps"]
    hv, bpm, nm = _geometry(info)
    mcux, mcuy, ri = info["mcux"], info["mcuy"], info["ri"] or nm
    sizes = [mcux * h * mcuy * v * 64 for (_, h, v, _) in comps]
    base = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    coef = np.zeros(base[-1], np.int16)
    if status is not None:                                        # refused: the status pass leaves every block empty
        return coef, rounds, CAUSES[status & 7]
    # k_jpeg_dc: running sum of the DC differences per component, modulo 2^16, restarted at every segment
    pred = [0, 0, 0]
    for b in range(nm * bpm):
        m, jj = divmod(b, bpm)
        if jj == 0 and m % ri == 0:
            pred = [0, 0, 0]
        c = 0 if jj < hv else 1 + jj - hv
        pred[c] = (pred[c] + ent[tab[b]]) & 0xFFFF
        ent[tab[b]] = pred[c]
    h0, v0 = comps[0][1], comps[0][2]
    for b in range(nm * bpm):
        m, jj = divmod(b, bpm)
        my, mx = divmod(m, mcux)
        if jj < hv:
            c, by, bx = 0, my * v0 + jj // h0, mx * h0 + jj % h0
        else:
            c, by, bx = 1 + jj - hv, my, mx
        o = base[c] + (by * mcux * comps[c][1] + bx) * 64
        for e in ent[tab[b]:tab[b + 1]]:
            coef[o + ((e >> 16) & 63)] = np.uint16(e & 0xFFFF).astype(np.int16)
    return coef, rounds, None


def entry_count(st):
    """(entries the stream() holds, the capacity derived from the scan's length)."""
    return st[1][-1], st[5]
