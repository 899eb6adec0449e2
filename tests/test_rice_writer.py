"""The symbol-level packet writer (tests/rice_writer.py) against the two CPU oracles and the synthetic encoder, and the premises
and oracle verdicts of every directed case of tests/tier_cases.py -- all without a GPU.  The writer is pinned by the oracles, not
by itself: a rule of its state machine that is changed (the 128 of the run symbol, the cap of k at rice_kmodifier) makes the
round trip below fail."""
import random

import numpy as np
import pytest

import rice_writer as rw
import tier_cases as tc


def random_symbols(rnd, cfg, rss, ricemod, n):
    cw = rw.ChannelWriter(cfg, rss, ricemod, n)
    while not cw.done:
        try:
            if cw.expects_run:
                cw.run(rnd.choice([0, 1, 2, 7, 8, 40, rnd.randrange(300)]), rnd.random() < 0.3)
            else:
                top = rnd.choice([2, 8, 200, 70000, 1 << rss])
                cw.value(rnd.randrange(cw.signmod, max(top, 2)), rnd.random() < 0.2)
        except rw.WriterError:     # a draw outside the domain (a history past int32, a value wider than its raw field): draw again
            cw.value(cw.signmod) if not cw.expects_run else cw.run(0)
    return cw.symbols


def expected(symbols, n, ss):
    return [rw.sign_extend(v, 32) if ss == 16 else rw.sign_extend(v, 24) for v in rw.expand(symbols, n)]


@pytest.mark.parametrize("ss", [16, 24])
@pytest.mark.parametrize("kb", [1, 8, 14, 16, 17, 33])
def test_random_symbols_round_trip_through_both_oracles(oracle, ss, kb):
    import alacfile_literal as lit

    rnd = random.Random(100 * kb + ss)
    for pb in (8, 40, 255):
        for ricemod in range(8):
            n = rnd.choice([1, 2, 33, rnd.randrange(1, 400), rnd.randrange(400, 4097)])
            cfg = (4096, ss, pb, 10, kb, 1)
            symbols = random_symbols(rnd, cfg, ss, ricemod, n)
            pkt, traces, _ = rw.write_packet(cfg, n, [rw.channel_header(ricemod=ricemod)], [symbols])
            want = expected(symbols, n, ss)
            st, pcm, ob, ns = oracle.decode_frame(cfg, pkt + bytes(16))
            assert (st, ns, ob) == (0, n, n * ss // 8) and pcm.tolist() == want, (cfg, ricemod, n)
            if len(symbols) <= 2000 and ricemod % 3 == 0:
                out, ret = lit.decode_packet(cfg, pkt)
                assert ret == ob and lit.canonical_from_reference_layout(out, n, ss, 1) == want, (cfg, ricemod, n)


@pytest.mark.parametrize("ss,kb,pb", [(16, 14, 40), (24, 14, 40), (16, 8, 255), (24, 17, 8), (16, 33, 40), (16, 1, 40)])
def test_canonical_streams_equal_the_synthetic_encoder_byte_for_byte(synth, ss, kb, pb):
    rnd = random.Random(ss + kb + pb)
    for ricemod in (0, 1, 4, 7):
        n = rnd.randrange(50, 900)
        # the history settles near 512 * dv, and its product with hist_mult has to stay inside int32: the amplitudes keep
        # 512 * dv * hist_mult below 2^31 (pb 255 with a large modifier: small values only), so that the writer refuses nothing
        hist_mult = ricemod * (pb // 4)
        cap = (1 << (ss - 1)) if hist_mult <= 40 else (1 << 31) // (512 * 2 * hist_mult) - 1
        amp = min(rnd.choice([1, 3, 40, 3000, 1 << (ss - 1)]), cap)
        res = [0 if rnd.random() < 0.4 else rnd.randrange(-amp, amp) for _ in range(n)]
        cfg = (4096, ss, pb, 10, kb, 1)
        symbols = rw.symbols_for_residuals(cfg, ss, ricemod, res)
        pkt, _, _ = rw.write_packet(cfg, n, [rw.channel_header(ricemod=ricemod)], [symbols])
        d = synth.packet_descs(1, n=n, max_samples_per_frame=4096, sample_size=ss, stereo=0, pred_order=0, ricemod=ricemod,
                               rice_history_mult=pb, rice_kmodifier=kb, mix_shift=0, mix_weight=0)
        assert synth.encode_packet(d, np.array(res, dtype=np.int32)) == pkt, (cfg, ricemod)


def _packets(g):
    return [(g.cfgs[g.cfg_idx[j]], g.packets[j], g.status[j], g.ns[j]) for j in range(len(g.packets))]


def check_group_on_both_oracles(oracle, g, literal_budget=2000):
    import alacfile_literal as lit

    for cfg, pkt, status, n in _packets(g):
        st, pcm, ob, ns = oracle.decode_frame(cfg, pkt + bytes(16))
        assert st == status and ns == n, (g.name, st, status)
        if n > literal_budget:
            continue               # the long ones: see test_long_cases_agree_on_a_truncated_copy
        if status:
            with pytest.raises(IndexError):
                lit.decode_packet(cfg, pkt)
            continue
        out, ret = lit.decode_packet(cfg, pkt)
        assert ret == ob and lit.canonical_from_reference_layout(out, n, cfg[1], cfg[5]) == pcm.tolist(), g.name


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_premises_and_oracle_status(oracle, name, stereo, is24):
    # the builder asserts the premise; every packet decodes with status 0 in the C oracle but the one that is there for a status
    for oc in tc.ORDER_CLASSES:
        g = tc.build(name, stereo, is24, oc)
        assert (max(g.ns) > 4096) == ((name, stereo, is24) in tc.OVER_4096_FRAMES), "tc.OVER_4096_FRAMES is out of date"
        b = g.batch()
        o = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"],
                                n_threads=8)
        assert o[3].tolist() == b["status"] and o[2].tolist() == [g.ns[j] for j in b["order"]], (name, oc)


@pytest.mark.parametrize("name", [c for c in tc.CASES if c not in ("h", "k_59", "k_34", "l")])
def test_short_cases_agree_in_both_oracles(oracle, name):
    check_group_on_both_oracles(oracle, tc.build(name, True, False, "second_launch"))
    check_group_on_both_oracles(oracle, tc.build(name, False, True, "first_launch"))


@pytest.mark.parametrize("name", ["h", "k_59", "k_34", "l"])
def test_long_cases_agree_on_a_truncated_copy(oracle, name):
    # every packet of the group with its own stream configuration, Rice modifiers and channel headers, its symbols cut to 600
    # samples (a hassize header): both oracles on the cut copy
    import alacfile_literal as lit

    g = tc.build(name, True, True, "two_taps")
    for j in range(8):
        cfg = g.cfgs[g.cfg_idx[j]]
        n = min(600, g.ns[j])
        hdr, syms = g.headers[j], []
        for ch, tr in zip(hdr, g.traces[j]):
            cw = rw.ChannelWriter(cfg, 25, ch["ricemod"], n)
            for t in tr:
                if cw.done:
                    break
                cw.value(t.value, t.escape) if t.kind == "v" else cw.run(t.value, t.escape)
            assert cw.done
            syms.append(cw.symbols)
        pkt, _, _ = rw.write_packet(cfg, n, hdr, syms, mix_shift=2, mix_weight=j % 3)
        st, pcm, ob, ns = oracle.decode_frame(cfg, pkt + bytes(16))
        out, ret = lit.decode_packet(cfg, pkt)
        assert st == 0 and ns == n and ret == ob, (name, j)
        assert lit.canonical_from_reference_layout(out, n, 24, 2) == pcm.tolist(), (name, j)


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", tc.FIR_KINDS)
def test_fir_case_premises_and_oracles(oracle, kind, stereo, is24):
    for block in tc.fir_blocks(kind):
        g = tc.build_fir(kind, stereo, is24, block)
        if block == 0:
            check_group_on_both_oracles(oracle, g)
        else:
            for cfg, pkt, status, n in _packets(g):
                assert oracle.decode_frame(cfg, pkt + bytes(16))[0] == 0


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("order_class", tc.ORDER_CLASSES)
@pytest.mark.parametrize("kind", tc.FIR_KINDS)
def test_fir_order_class_premises_and_oracles(oracle, kind, order_class, stereo, is24):
    # the builder asserts the premise and the routing facts (every order inside its class) per class
    for block in tc.fir_blocks(kind, order_class):
        g = tc.build_fir(kind, stereo, is24, block, order_class)
        if block == 0:
            check_group_on_both_oracles(oracle, g)
        else:
            for cfg, pkt, status, n in _packets(g):
                assert oracle.decode_frame(cfg, pkt + bytes(16))[0] == 0


def test_the_four_tap_threshold_is_the_kernels():
    # Group.embed builds launches of L16_MAX_GROUPS + 1 groups so that orders above 16 take the four-taps-per-lane step
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alac.net_amd", "csrc", "alac_kernels.hip")
    with open(src) as f:
        found = re.findall(r"^#define\s+ALAC_L16_MAX_GROUPS\s+(\d+)", f.read(), re.M)
    assert found == [str(tc.L16_MAX_GROUPS)], found
    assert tc.EMBED_PACKETS == 8 * 256 + 8 == 2056


@pytest.mark.parametrize("stereo,is24", [(True, False), (False, True)])
def test_embedded_batch_layout_and_oracle(oracle, stereo, is24):
    # the group at group 0, in the middle (rolled by 3) and last (rolled by 5), filler everywhere else; the oracle takes it all
    g = tc.build_fir("drift", stereo, is24, 0, "second_launch")
    filler = tc.embed_filler(stereo, is24)
    b = g.embed(filler)
    n = tc.EMBED_PACKETS
    assert len(b["offsets"]) == len(b["sizes"]) == len(b["cfg_idx"]) == len(b["status"]) == n
    pkt = lambda i: bytes(b["blob"][int(b["offsets"][i]):int(b["offsets"][i]) + int(b["sizes"][i])])
    mid = 8 * (tc.EMBED_GROUPS // 2)
    assert [i for i, _ in b["order"]] == list(range(8)) + list(range(mid, mid + 8)) + list(range(n - 8, n))
    assert [j for _, j in b["order"]] == list(range(8)) + [(k + 3) % 8 for k in range(8)] + [(k + 5) % 8 for k in range(8)]
    own = dict(b["order"])
    for i in range(n):
        assert pkt(i) == (g.packets[own[i]] if i in own else filler.packets[i % 8])
    assert b["slot_ints"] == 160 * (2 if stereo else 1) + 8 and max(filler.ns) <= 32
    o = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"],
                            n_threads=8)
    assert o[3].tolist() == b["status"]
    assert o[2].tolist() == [g.ns[own[i]] if i in own else filler.ns[i % 8] for i in range(n)]


def test_fir_replay_equals_the_oracle_predictor(oracle):
    rnd = random.Random(7)
    for order in (1, 2, 5, 8, 13, 30):
        for rss, q in ((16, 0), (17, 9), (24, 15), (25, 1)):
            top = (1 << (rss - 1)) - 1
            res = [rnd.randrange(-top, top) >> rnd.choice([0, 8, rss - 3]) for _ in range(120)]
            coefs = [rnd.randrange(-32768, 32768) for _ in range(order)]
            out, peak, _, _ = tc.fir_replay(res, rss, coefs, q)
            buf, cf = oracle.predictor(res, rss, coefs, q)
            assert buf.tolist() == out and peak >= int(np.abs(cf).max())
