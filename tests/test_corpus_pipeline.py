"""What the one crop pipeline of Corpus must keep and no other test asserts: a resident corpus from PCM never fetches its
packet tables for a step, whatever the kind of crop; every kind of crop refuses a closed corpus; and the public K and S are
those of the module-level functions, with a source window per file where the rates differ."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, L, TARGET = 4, 1000, 16000
RATES = (44100, 48000)
LENGTHS = [12000, 11111]        # two files of about three packets of 4096 frames


@pytest.fixture(scope="module")
def material():
    """(pcm float32 [2, 2, 12000] on the device, the two files of it as M4A bytes at 44100 Hz, the same two at 44100 and 48000)"""
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    pcm = torch.stack([signal(torch, RATES[0], max(LENGTHS), 70 + f) for f in range(2)])

    def files(rates):
        out = []
        for f, rate in enumerate(rates):
            buf = io.BytesIO()
            pkg.save_batch([buf], pcm[f:f + 1], LENGTHS[f:f + 1], rate)
            out.append(buf.getvalue())
        return out

    return pcm, files((RATES[0], RATES[0])), files(RATES)


def calls(corpus, rate):
    """The four kinds of call, on device indices and unchecked; `rate`: the corpus's own"""
    import torch

    from alac.net_amd.features import LogMel

    files = torch.tensor([0, 1, 1, 0], device="cuda")
    offs = torch.tensor([0, 17, 2500, 3000], device="cuda")
    return {"native": lambda: corpus.crops(files, offs, L, check=False),
            "sample_rate": lambda: corpus.crops(files, offs, L, check=False, sample_rate=TARGET),
            "mono": lambda: corpus.crops(files, offs, L, check=False, mono=True),
            "features": lambda: corpus.crops(files, offs, L, check=False, features=LogMel(rate))}


def test_a_resident_corpus_from_pcm_reads_no_packet_table_for_any_kind_of_crop(material):
    import torch

    import alac.net_amd as pkg

    pcm, _, mixed_files = material
    with pkg.Corpus.from_pcm(pcm, LENGTHS, RATES[0]) as corpus:
        assert corpus.tier_bytes[1] == 0
        for name, call in calls(corpus, RATES[0]).items():
            out, lengths = call()
            assert out.shape[0] == B and (lengths > 0).all(), name
            assert "pkt_size" not in corpus._host and "pkt_offset" not in corpus._host, name
    with pkg.Corpus(mixed_files, mixed_rates=True) as corpus:
        assert corpus.sample_rate is None
        before = set(corpus._host)
        files, offs = torch.tensor([0, 1, 1, 0], device="cuda"), torch.tensor([0, 17, 2500, 3000], device="cuda")
        out, lengths = corpus.crops(files, offs, L, check=False, sample_rate=TARGET)
        assert out.shape == (B, 2, L) and (lengths == L).all()
        assert set(corpus._host) == before


def test_every_kind_of_crop_refuses_a_closed_corpus(material):
    import alac.net_amd as pkg

    pcm, _, mixed_files = material
    corpus = pkg.Corpus.from_pcm(pcm, LENGTHS, RATES[0])
    corpus.close()
    for name, call in calls(corpus, RATES[0]).items():
        with pytest.raises(pkg.AlacGpuError, match="the corpus is closed"):
            call()
    corpus = pkg.Corpus(mixed_files, mixed_rates=True)
    corpus.close()
    with pytest.raises(pkg.AlacGpuError, match="the corpus is closed"):
        corpus.crops([0, 1], [0, 0], L, sample_rate=TARGET)


def test_the_public_bounds_are_the_module_level_functions(material):
    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_table, source_window

    _, same_files, mixed_files = material
    with pkg.Corpus(same_files) as corpus, pkg.Corpus(same_files, hbm_bytes=0) as tiered:
        h = corpus._host
        assert corpus.entries_per_crop(L, sample_rate=TARGET) == corpus.entries_per_crop(L) == \
            max(pkg.entries_per_crop(h["pkt_end"], h["file_first"], L), 1)
        assert tiered.tier_bytes[0] == 0 and tiered.tier_bytes[1] > 0
        assert tiered.stage_bytes_per_crop(L, sample_rate=TARGET) == tiered.stage_bytes_per_crop(L) == \
            pkg.stage_bytes_per_crop(h["pkt_size"], h["pkt_end"], h["file_first"], L) > 0
    with pkg.Corpus(mixed_files, mixed_rates=True) as corpus:
        Ls = np.array([source_window(0, L, *resample_table(rate, TARGET)[:3])[1] for rate in RATES], dtype=np.int64)
        assert Ls[0] != Ls[1]
        h = corpus._host
        assert corpus.entries_per_crop(L, sample_rate=TARGET) == max(pkg.entries_per_crop(h["pkt_end"], h["file_first"], Ls), 1)
        assert corpus.stage_bytes_per_crop(L, sample_rate=TARGET) == \
            pkg.stage_bytes_per_crop(h["pkt_size"], h["pkt_end"], h["file_first"], Ls) > 0
