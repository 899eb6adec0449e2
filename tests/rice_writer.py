"""Symbol-level writer of compressed ALAC packets (tests only, pure Python, on top of bitpack.pack).

Where the synthetic encoder turns PCM into whatever symbols its predictor leaves, this module puts CHOSEN symbols into a packet:
per channel a list of Value(dv, escape) and Run(length, escape).  It walks the decoder's entropy state machine as
AlacFile.cs:193-252 states it -- written from that text, sharing no code with oracle/, synth/ or the kernels -- and returns the
packet bytes and a trace: per symbol its k, unary prefix, value, whether it was an escape code, its bits, the history after it and
its sample index.  The trace is what lets a test state, on the CPU, that its input really sits on the edge it claims.

Domain: rice_kmodifier >= 1 (the GPU library refuses 0), histories that stay inside int32 and non-negative (anything else raises).
"""
import copy
from collections import namedtuple

from bitpack import pack

Value = namedtuple("Value", "dv escape", defaults=(False,))
Run = namedtuple("Run", "length escape", defaults=(False,))
# kind 'v' / 'r'; x is the number of ones read (9: an escape code); bitpos is the symbol's first bit, counted from the start of
# the channel's Rice stream (write_packet adds the packet's own offset); index is the sample the symbol belongs to (a run symbol:
# the value it follows); hist is the history after the symbol (0 after a run symbol).
Sym = namedtuple("Sym", "kind index k x value escape bits bitpos hist")

RICE_THRESHOLD = 8


class WriterError(ValueError):
    pass


def clz(x):
    """CountLeadingZeros, :170-191: 32-bit clz, but 40 for 0 (and 0 for a negative int)."""
    if x == 0:
        return 40
    if x < 0:
        return 0
    return 32 - x.bit_length()


def fold(dv):
    """:225-226: the residual a decoded value stands for."""
    h = (dv + 1) // 2
    return -h if dv & 1 else h


def unfold(r):
    return 2 * r if r >= 0 else -2 * r - 1


def sign_extend(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


class ChannelWriter:
    """The Rice stream of one channel, symbol by symbol.  cfg = (max_spf, sample_size, pb, mb, kb, channels)."""

    def __init__(self, cfg, rss, ricemodifier, n):
        _, _, pb, mb, kb, _ = cfg
        if kb < 1:
            raise WriterError("rice_kmodifier 0 is outside the writer's domain")
        self.rss, self.n, self.kb = rss, n, kb
        self.hist_mult = ricemodifier * (pb // 4)            # :483 / :643
        self.run_mask = ((1 << (kb & 31)) - 1) & 0xFFFFFFFF  # (1 << kb) - 1 with C#'s five-bit shift count
        self.history = mb
        self.index = 0                                       # outputCount
        self.signmod = 0
        self.expects_run = False
        self.gentle = True                                   # level_dv / hold never pick a value that needs an escape code
        self.fields, self.trace, self.symbols, self.bitpos = [], [], [], 0

    def clone(self):
        c = copy.copy(self)
        c.fields, c.trace, c.symbols = list(self.fields), list(self.trace), list(self.symbols)
        return c

    @property
    def done(self):
        return self.index >= self.n and not self.expects_run

    # ---- the decoder's parameters for the next symbol --------------------------------------------------------------------
    def k(self):
        """:221-222, for the next value"""
        initial = 31 - self.kb - clz((self.history >> 9) + 3)
        return initial + self.kb if initial < 0 else self.kb

    def run_k(self):
        """:234, for the run symbol that follows a history < 128"""
        return clz(self.history) + (self.history + 16) // 64 - 24

    # ---- one symbol (the inverse of EntropyDecodeValue, :193-212) -------------------------------------------------------------
    def _put(self, code, k, modulus, raw_bits, escape):
        if code < 0:
            raise WriterError("a pending signModifier needs dv >= 1")
        x, rem = (code // modulus, code % modulus) if modulus > 0 else (RICE_THRESHOLD + 1, 0)
        if escape or x > RICE_THRESHOLD:
            if code >> raw_bits:
                raise WriterError(f"{code} does not fit the {raw_bits} raw bits of an escape code")
            f = [(9, 0x1FF), (raw_bits, code)]
            x, escape = 9, True
        elif k == 1:                                   # the early return: no extra bit is read
            if rem:
                raise WriterError("k == 1 with a remainder")
            f = [(x + 1, ((1 << x) - 1) << 1)]
        elif rem == 0:                                 # k bits read, value <= 1, one bit handed back: k - 1 zeros
            f = [(x + 1, ((1 << x) - 1) << 1), (k - 1, 0)]
        else:
            if rem + 1 >= (1 << k):
                raise WriterError("remainder does not fit k bits")
            f = [(x + 1, ((1 << x) - 1) << 1), (k, rem + 1)]
        f = [t for t in f if t[0] > 0]
        bits = sum(t[0] for t in f)
        self.fields += f
        start = self.bitpos
        self.bitpos += bits
        return x, escape, bits, start

    def value(self, dv, escape=False):
        if self.expects_run:
            raise WriterError(f"sample {self.index}: the decoder reads a run symbol here (history {self.history} < 128)")
        if self.index >= self.n:
            raise WriterError("more values than samples")
        k = self.k()
        if k < 1 or k > 16:
            raise WriterError(f"k {k} outside 1..16")
        if dv > 0xFFFF:                                # :229
            h = 0xFFFF
        else:
            h = self.history + dv * self.hist_mult - ((self.history * self.hist_mult) >> 9)
        if not 0 <= h < 1 << 31 or h * self.hist_mult >= 1 << 31:
            raise WriterError("history (or its product with the multiplier) leaves int32: outside the supported domain")
        x, esc, bits, start = self._put(dv - self.signmod, k, (1 << k) - 1, self.rss, escape)
        self.signmod = 0
        self.history = h
        self.trace.append(Sym("v", self.index, k, x, dv, esc, bits, start, h))
        self.symbols.append(Value(dv, escape))
        if h < 128 and self.index + 1 < self.n:        # :231
            self.signmod = 1
            self.expects_run = True
        self.index += 1
        return self

    def run(self, length, escape=False):
        if not self.expects_run:
            raise WriterError(f"sample {self.index}: no run symbol is read here")
        k = self.run_k()
        modulus = ((1 << k) - 1) & self.run_mask
        if k < 2 or k > 16:
            raise WriterError(f"run k {k}")
        if length > 0xFFFF:
            raise WriterError("a run symbol holds at most 16 bits")
        x, esc, bits, start = self._put(length, k, modulus, 16, escape)
        self.trace.append(Sym("r", self.index - 1, k, x, length, esc, bits, start, 0))
        self.symbols.append(Run(length, escape))
        self.index += length                           # :244 (zeros past the packet's end: the decoder's business)
        self.history = 0                               # :248
        self.expects_run = False
        return self

    # ---- steering ------------------------------------------------------------------------------------------------------------
    def history_after(self, dv):
        return 0xFFFF if dv > 0xFFFF else self.history + dv * self.hist_mult - ((self.history * self.hist_mult) >> 9)

    def dv_for_history(self, h):
        """the dv that leaves the history at exactly h (solve :229), or None when no dv does"""
        if h == 0xFFFF and self.signmod <= 0x10000:
            cand = [0x10000]
        else:
            cand = []
        if self.hist_mult > 0:
            num = h - self.history + ((self.history * self.hist_mult) >> 9)
            if num % self.hist_mult == 0:
                cand.insert(0, num // self.hist_mult)
        elif h == self.history:
            cand.insert(0, self.signmod)
        for dv in cand:
            if self.signmod <= dv and (dv <= 0xFFFF or h == 0xFFFF) and self.history_after(dv) == h:
                return dv
        return None

    def dv_with_prefix(self, x, rem=0):
        """a dv whose canonical code has x ones (x = 9: the canonical escape code) at the current k"""
        return x * ((1 << self.k()) - 1) + rem + self.signmod

    def level_dv(self, level):
        """the dv that brings the history as close to `level` as one value can"""
        if self.hist_mult == 0:
            return self.signmod
        num = level - self.history + ((self.history * self.hist_mult) >> 9)
        dv = min(max((num + self.hist_mult // 2) // self.hist_mult, self.signmod), 0xFFFF)
        return min(dv, 8 * ((1 << self.k()) - 1) - 1 + self.signmod) if self.gentle else dv

    def hold(self, level, m, floor=128):
        """m values that keep the history near `level` (and at or above `floor`: no run symbol)"""
        for _ in range(m):
            dv = self.level_dv(level)
            while self.hist_mult and self.history_after(dv) < floor:
                dv += 1
            self.value(dv)
        return self

    def hold_to(self, index, level, floor=128):
        if index < self.index:
            raise WriterError(f"already past sample {index}")
        return self.hold(level, index - self.index, floor)

    def steer_at(self, index, goal, level, max_path=20, span=24):
        """Values up to and including sample `index`, whose value leaves a history with goal(h) true -- no run symbol on the
        way.  Holds `level` first, then takes the shortest path of values that gets there."""
        longest = min(max_path, index - self.index + 1)
        for lv in range(level, level + 8):               # (paths are sparse: a few levels to hold before them)
            c = self.clone().hold_to(index - longest + 1, lv)
            for plen in range(longest, 0, -1):           # c stands at the sample where a path of plen values starts
                path = c._path(plen, goal, span)
                if path is not None:
                    self.hold_to(index - plen + 1, lv)
                    for dv in path:
                        self.value(dv)
                    return self
                if plen > 1:
                    c.hold(lv, 1)
        raise WriterError(f"no path to the goal at sample {index}")

    def _path(self, plen, goal, span):
        # breadth first over histories, plen values exactly
        hm = self.hist_mult
        frontier = {self.history: []}
        for step in range(plen):
            last = step == plen - 1
            nxt = {}
            for h, p in frontier.items():
                lo = self.signmod if step == 0 else 0
                for dv in range(lo, lo + (span if last else 4)):     # small steps on the way, any value at the end
                    h2 = h + dv * hm - ((h * hm) >> 9)
                    if last:
                        if goal(h2):
                            return p + [dv]
                    elif 128 <= h2 < 8192 and h2 not in nxt:
                        nxt[h2] = p + [dv]
            frontier = nxt
        return None


def symbols_for_residuals(cfg, rss, ricemodifier, residuals):
    """The canonical symbol list of a residual sequence: every value coded as the decoder's state asks, every zero run maximal
    (what an encoder would write)."""
    n = len(residuals)
    cw = ChannelWriter(cfg, rss, ricemodifier, n)
    i = 0
    while i < n:
        cw.value(unfold(int(residuals[i])))
        i += 1
        if cw.expects_run:
            z = 0
            while i + z < n and residuals[i + z] == 0 and z < 0xFFFF:
                z += 1
            cw.run(z)
            i += z
    return cw.symbols


def expand(symbols, n=None):
    """the residuals a symbol list stands for: values folded, runs expanded (cut at n)"""
    out = []
    for s in symbols:
        if isinstance(s, Value):
            out.append(fold(s.dv))
        else:
            out.extend([0] * s.length)
    return out if n is None else (out + [0] * n)[:n]


def channel_header(order=0, coefs=(), quant=9, ricemod=4, pred_type=0):
    coefs = list(coefs)
    if len(coefs) != order:
        raise WriterError("one coefficient per tap")
    return dict(order=order, coefs=coefs, quant=quant, ricemod=ricemod, pred_type=pred_type)


def write_packet(cfg, n, channels, symbols, hassize=None, ub=0, mix_shift=0, mix_weight=0, shift_bytes=None, element=None,
                 end_tag=True, slack=0):
    """One compressed packet.  channels: a channel_header() per channel of the element (one or two); symbols: a list of Value /
    Run per channel.  Returns (bytes, traces, nbits): a trace per channel with packet-relative bit positions, and the bits written
    before the END tag and the padding."""
    max_spf, sample_size = cfg[0], cfg[1]
    stereo = len(channels) == 2
    element = (1 if stereo else 0) if element is None else element
    hassize = (n != max_spf) if hassize is None else hassize
    rss = sample_size - 8 * ub + (1 if stereo else 0)   # :454 / :596
    f = [(3, element), (4, 0), (12, 0), (1, int(hassize)), (2, ub), (1, 0)]
    if hassize:
        f.append((32, n))
    f += [(8, mix_shift), (8, mix_weight)] if stereo else [(8, 0), (8, 0)]
    for ch in channels:
        f += [(4, ch["pred_type"]), (4, ch["quant"]), (3, ch["ricemod"]), (5, ch["order"])]
        f += [(16, c & 0xFFFF) for c in ch["coefs"]]
    if ub:
        for i in range(n):
            for c in range(len(channels)):
                f.append((8 * ub, shift_bytes[c][i] if shift_bytes else 0))
    pos = sum(t[0] for t in f)
    traces = []
    for ch, syms in zip(channels, symbols):
        cw = ChannelWriter(cfg, rss, ch["ricemod"], n)
        for s in syms:
            if isinstance(s, Value):
                cw.value(s.dv, s.escape)
            else:
                cw.run(s.length, s.escape)
        if not cw.done:
            raise WriterError(f"the symbols end at sample {cw.index} of {n}" + (", a run symbol short" if cw.expects_run else ""))
        f += cw.fields
        traces.append([t._replace(bitpos=t.bitpos + pos) for t in cw.trace])
        pos += cw.bitpos
    if end_tag:
        f.append((3, 7))
    return pack(f, slack=slack), traces, pos
