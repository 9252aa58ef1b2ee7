"""The index arithmetic of wb_gram_fused_kernel (cellregmap_amd/csrc/wb_gram_fused.hip) in numpy: the LDS table
(wb_gram_fused_layout), what every lane of every LDS-DMA instruction reads and where it lands, the walk over the donors in
chunks that end at multiples of four positions, the columns the rotated S of a donor is written to, and the fragment reads of
the rotation and of the Gram.  LDS is an array of NaN that only the writes of the kernel fill, global memory is one flat
array with the operands at the alignments the launch checks, and every read is bounds-checked against the buffer it belongs
to -- an address that is off by a row, a chunk or a donor shows as a NaN in Gw or as an assertion here, not as a fault on a
device.  `fused_gw` returns Gw and the donor sums of one variant; tests/test_wb_gram_fused_prototype_cpu.py holds them
against the two launches' arithmetic written plainly."""
import numpy as np

WF_UW = 56
GROUP = 4


def pair(lo, hi, k0):
    return lo * k0 - lo * (lo - 1) // 2 + (hi - lo)


def layout(k0, KT, ldp):
    KS = (k0 + 3) // 4
    L = dict(urows=4 * KS, UW=WF_UW, RS=(k0 + 4) | 2, nP=ldp // 128, rows_o=KT - k0)
    L["nU"] = (L["urows"] * (L["UW"] // 2) + 63) // 64
    L["nO"] = (L["rows_o"] * (L["RS"] // 2) + 63) // 64
    L["off_P"] = k0 * L["RS"] + L["nO"] * 128
    L["off_U"] = L["off_P"] + L["nP"] * 128
    L["off_S0"] = L["off_U"] + L["nU"] * 128
    L["off_d"] = L["off_S0"] + 128
    L["off_rp"] = L["off_d"] + 64
    L["total"] = L["off_rp"] + ((L["rows_o"] + 1) & ~1)
    return L


def chunk(d, k0, donors):
    """(start, end, c0, lim): positions [start, end) of donor d's chunk at columns c0 ..; data up to position lim."""
    ptot = donors * k0
    start = (k0 * d) & ~3
    end = (k0 * (d + 1)) & ~3 if d + 1 < donors else (ptot + 3) & ~3
    return start, end, 2 - (k0 * d - start), min(end, ptot)


class Global:
    """Flat global memory: named buffers at 16-byte boundaries, NaN between them; reads know their buffer."""

    def __init__(self):
        self.mem = np.full(0, np.nan)
        self.spans = {}

    def add(self, name, array):
        base = (self.mem.size + 1) & ~1
        flat = np.asarray(array, float).ravel()
        self.mem = np.concatenate([self.mem, np.full(base - self.mem.size, np.nan), flat, np.full(3, np.nan)])
        self.spans[name] = (base, base + flat.size)
        return base

    def read16(self, name, addr):
        lo, hi = self.spans[name]
        assert addr % 2 == 0, ("a 16-byte load from an odd element", name, addr - lo)
        assert lo <= addr and addr + 2 <= hi, ("load outside its buffer", name, addr - lo, hi - lo)
        return self.mem[addr:addr + 2]


def fused_gw(P, U, rows, S0, k0, c, ratio, has_A=True, splits=1):
    """P [donors][ldp] the variant's pair products; U [donors][k2pad][128]; rows [KT - k0][ldr] the other operand rows in the
    Gram's order (W, gx, y, E1), zero past donors k0; S0 [ldr].  Returns (Gw [KT][KT], Psum [splits][npair], stats)."""
    donors, ldp = P.shape
    k2pad, ldu = U.shape[1:]
    rows_o, ldr = rows.shape
    KT = k0 + rows_o
    npair, KS, JT = k0 * (k0 + 1) // 2, (k0 + 3) // 4, (k0 + 15) // 16
    L = layout(k0, KT, ldp)
    RS, UW = L["RS"], L["UW"]
    assert k0 % 2 == 0 and ldp % 128 == 0 and ldp >= npair and k2pad >= 4 * KS and RS <= 64
    ptot = donors * k0
    G = Global()
    gP, gU, gR, gS0, gZ = G.add("P", P), G.add("U", U), G.add("rows", rows), G.add("S0", S0), G.add("zeros", np.zeros(128))
    lds = np.full(L["total"], np.nan)
    img = lds[:L["off_P"]]
    lds[:k0 * RS] = 0.0
    rowp = [gR + t * ldr for t in range(rows_o)]
    stats = dict(dma_instructions=0, lds_doubles=L["total"])

    def dma(dest, sources):
        """One wave-instruction: lane l writes the 16 bytes `sources[l]` = (buffer, element address) at dest + 2 l."""
        assert dest % 2 == 0 and dest + 128 <= L["total"]
        for lane, (name, addr) in enumerate(sources):
            lds[dest + 2 * lane:dest + 2 * lane + 2] = G.read16(name, addr)
        stats["dma_instructions"] += 1

    def issue_pus(d):
        start, end, c0, lim = chunk(d, k0, donors)
        for I in range(L["nP"]):
            dma(L["off_P"] + 128 * I, [("P", gP + d * ldp + 128 * I + 2 * lane) for lane in range(64)])
        for I in range(L["nU"]):
            src = []
            for lane in range(64):
                u = 64 * I + lane
                k, cu = divmod(u, UW // 2)
                src.append(("U", gU + d * k2pad * ldu + (k * ldu + 2 * cu if k < L["urows"] else 0)))
            dma(L["off_U"] + 128 * I, src)
        src = []
        for lane in range(64):
            col = 2 * lane
            inside = col >= c0 and start - c0 + col < lim
            src.append(("S0", gS0 + start - c0 + col) if inside else ("zeros", gZ))
        dma(L["off_S0"], src)

    def issue_others(d):
        start, end, c0, lim = chunk(d, k0, donors)
        shift = start - c0
        for I in range(L["nO"]):
            src = []
            for lane in range(64):
                t, cu = divmod(64 * I + lane, RS // 2)
                col = 2 * cu
                inside = t < rows_o and col >= c0 and shift + col < lim
                src.append(("rows", rowp[t] + shift + col) if inside else ("zeros", gZ))
            dma(k0 * RS + 128 * I, src)

    def row_off(R):
        return (R if R < KT else 0) * RS

    NTL = (KT + 15) // 16
    Gw = np.zeros((16 * NTL, 16 * NTL))
    psum, Psum = np.zeros(npair), np.zeros((splits, npair))
    per, split = (donors + splits - 1) // splits, 0
    issue_pus(0)
    issue_others(0)
    for d in range(donors):
        start, end, c0, lim = chunk(d, k0, donors)
        Pl, Ul = lds[L["off_P"]:L["off_P"] + ldp], lds[L["off_U"]:]
        # rotation phase
        s = ratio * lds[L["off_S0"]:L["off_S0"] + RS]
        lds[L["off_d"]:L["off_d"] + RS] = s / (1.0 + s)
        psum += Pl[:npair]
        if d + 1 == donors or d + 1 == (split + 1) * per:
            Psum[split], psum = psum, np.zeros(npair)
            split += 1
        if has_A:
            jcut = end - k0 * d
            for w in range(JT):
                A = np.zeros((16, 16 * JT))
                for ks in range(KS):
                    for lq in range(4):
                        k = 4 * ks + lq
                        a = np.array([Pl[pair(min(k, i), max(k, i), k0)] if k < k0 and i < k0 else Pl[0]
                                      for i in range(16 * w, 16 * w + 16)])
                        bfrag = Ul[k * UW:k * UW + 16 * JT]          # (columns past k0: whatever follows in LDS, never stored)
                        A += np.outer(a, bfrag)
                for r in range(16 * w, min(16 * w + 16, k0)):
                    for j in range(k0):
                        col = j + 2 if j < jcut else j - jcut
                        assert 0 <= col < RS
                        img[r * RS + col] = A[r - 16 * w, j]
        # (barrier) the next donor's P, Psi and S0 go out, then the Gram over the chunk's columns
        if d + 1 < donors:
            issue_pus(d + 1)
        dw = lds[L["off_d"]:L["off_d"] + RS]
        nks = (end - start) // GROUP
        assert c0 + GROUP * nks <= RS
        for ks in range(nks):
            cols = np.arange(c0 + GROUP * ks, c0 + GROUP * ks + GROUP)
            frag = np.array([[img[row_off(R) + col] for col in cols] for R in range(16 * NTL)])
            Gw += frag @ (frag * dw[cols]).T
        if d + 1 < donors:
            issue_others(d + 1)
    return Gw[:KT, :KT], Psum, stats
