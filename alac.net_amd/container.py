"""MP4/M4A demuxer -> batch feeder, and the `AlacContext` session surface (SURVEY.md section 8(f) rows 1,
2 and 4: the callers and the on-disk format on the input side of the decode path).

Host-side Python mirror of the reference's L1a/L2 layers, written from their behaviour:
  * `QtMovieT.ReadHeader` (ALACDecoder/QTMovieT.cs:51-109 and the atom readers :111-752) -> `DemuxResT`
    (DemuxResT.cs:22-34): ALACSpecificConfig in CodecData, packet sizes from stsz, durations from stts,
    chunk tables from stsc/stco.
  * `AlacContext` (ALACDecoder/AlacContext.cs:20-338): same public members -- GetSampleRate/NumChannels/
    BitsPerSample/BytesPerSample/NumSamples, Read(buffer), SetPosition(position), LastSampleNumber, Dispose --
    plus the batch entry point `ReadBatch`.  `Read` keeps the reference's contract (one packet per call,
    little-endian PCM bytes) but serves from batches decoded on the GPU through the C ABI: the next K packets
    are pre-read with the sizes the demuxer already holds and submitted in ONE alacgpu_decode_batch call.
Reference quirks kept on purpose: only moov-before-mdat files load (QTMovieT.cs:746 compares Seek()'s return,
the new position, with 0); stts is capped at 16 entries (DemuxResT.cs:27); the post-seek sample offset is
applied to the int[] buffer before formatting, so for 24-bit streams it is off by a factor 3
(AlacContext.cs:200-202,:284-286).
"""
import io
import os
import struct

import numpy as np

from . import MAX_FRAME, AlacGpuContext, _raise_reference_exception, cfg_from_codec_data, expand_reference_layout, format_samples

MDAT_NONE, MDAT_OK, MDAT_NO_VALID_SAVED_POS, MDAT_CANNOT_SEEK = 0, 1, 2, 3


def _fourcc(s):
    return struct.unpack(">I", s.encode("ascii"))[0]


class DemuxResT:
    """DemuxResT.cs:22-34"""

    def __init__(self):
        self.FormatRead = 0
        self.NumChannels = 0
        self.SampleSize = 0
        self.SampleRate = 0
        self.Format = 0
        self.TimeToSample = []          # (SampleCount, SampleDuration), at most 16 entries
        self.NumTimeToSamples = 0
        self.SampleByteSize = np.zeros(0, dtype=np.int64)
        self.CodecDataLength = 0
        self.CodecData = [0] * 1024
        self.Stco = []
        self.Stsc = []                  # (FirstChunk, SamplesPerChunk, SampleDescriptionIndex)
        self.MdatLen = 0


class _Stream:
    """MyStream.cs:14-115: big-endian reads over a seekable binary stream."""

    def __init__(self, f):
        self.f = f
        pos = f.tell()
        f.seek(0, io.SEEK_END)
        self.length = f.tell()
        f.seek(pos)

    @property
    def EOF(self):
        return self.f.tell() >= self.length

    @property
    def Position(self):
        return self.f.tell()

    def _rd(self, n):
        b = self.f.read(n)
        if len(b) < n:
            b = b + bytes(n - len(b))
        return b

    def ReadUint32(self):  # returned as a signed int in the reference (MyStream.cs:54)
        return struct.unpack(">i", self._rd(4))[0]

    def ReadUint16(self):
        return struct.unpack(">H", self._rd(2))[0]

    def ReadUint8(self):
        return self._rd(1)[0]

    def Read(self, n):
        return self._rd(n)

    def Skip(self, n):
        self.f.seek(n, io.SEEK_CUR)

    def Seek(self, pos):
        self.f.seek(pos)
        return self.f.tell()


class QtMovieT:
    """Atom walker with the reference's acceptance rules (QTMovieT.cs)."""

    def __init__(self, stream, res):
        self.s = stream
        self.res = res
        self.saved_mdat_pos = -1

    def ReadHeader(self):  # QTMovieT.cs:51-109
        found_moov = found_mdat = 0
        while True:
            chunk_len = self.s.ReadUint32()
            if self.s.EOF:
                return MDAT_NONE
            chunk_id = self.s.ReadUint32()
            if chunk_id == _fourcc("ftyp"):
                self._ftyp(chunk_len)
            elif chunk_id == _fourcc("moov"):
                if not self._container(chunk_len, "moov"):
                    return MDAT_NONE
                if found_mdat:
                    return self._set_saved_mdat()
                found_moov = 1
            elif chunk_id == _fourcc("mdat"):
                self._mdat(chunk_len, 0 if found_moov else 1)
                if found_moov:
                    return MDAT_OK
                found_mdat = 1
            elif chunk_id in (_fourcc("free"), _fourcc("junk")):
                self.s.Skip(chunk_len - 8)
            else:
                return MDAT_NONE  # unknown top-level atom (:103-107)

    def _ftyp(self, chunk_len):  # :111-132
        remaining = chunk_len - 8
        typ = self.s.ReadUint32()
        remaining -= 4
        if typ != _fourcc("M4A "):
            return
        self.s.ReadUint32()
        remaining -= 4
        while remaining != 0:
            self.s.ReadUint32()
            remaining -= 4

    _CHILDREN = {
        # container: {child: handler}; anything else makes the parse fail, as in the reference
        "moov": {"mvhd": "skip", "trak": "trak", "udta": "skip", "elst": "skip", "iods": "skip", "free": "skip"},
        "trak": {"tkhd": "skip", "mdia": "mdia", "edts": "skip"},
        "mdia": {"mdhd": "skip", "hdlr": "skip", "minf": "minf"},
        "stbl": {"stsd": "stsd", "stts": "stts", "stsz": "stsz", "stsc": "stsc", "stco": "stco"},
    }

    def _container(self, chunk_len, kind):  # ReadChunkMoov/Trak/Media/Stbl (:668,:135,:333,:179)
        remaining = chunk_len - 8
        table = self._CHILDREN[kind]
        while remaining != 0:
            sub_len = self.s.ReadUint32()
            if sub_len <= 1 or sub_len > remaining:
                return 0
            sub_id = self.s.ReadUint32()
            name = struct.pack(">i", sub_id).decode("latin1")
            h = table.get(name)
            if h is None:
                return 0
            if h == "skip":
                self.s.Skip(sub_len - 8)
            elif h in ("trak", "mdia"):
                if not self._container(sub_len, h):
                    return 0
            elif h == "minf":
                if not self._minf(sub_len):
                    return 0
            elif h == "stsd":
                if not self._stsd():
                    return 0
            elif h == "stts":
                self._stts(sub_len)
            elif h == "stsz":
                self._stsz(sub_len)
            elif h == "stsc":
                self.s.Skip(4)
                n = self.s.ReadUint32()
                self.res.Stsc = [(self.s.ReadUint32(), self.s.ReadUint32(), self.s.ReadUint32()) for _ in range(n)]
            elif h == "stco":
                self.s.Skip(4)
                n = self.s.ReadUint32()
                self.res.Stco = [self.s.ReadUint32() for _ in range(n)]
            remaining -= sub_len
        return 1

    def _minf(self, chunk_len):  # :258-331: smhd (16 bytes) then dinf then stbl, in this order
        remaining = chunk_len - 8
        if self.s.ReadUint32() != 16:
            return 0
        if self.s.ReadUint32() != _fourcc("smhd"):
            return 0
        self.s.Skip(8)
        remaining -= 16
        dinf = self.s.ReadUint32()
        if self.s.ReadUint32() != _fourcc("dinf"):
            return 0
        self.s.Skip(dinf - 8)
        remaining -= dinf
        stbl = self.s.ReadUint32()
        if self.s.ReadUint32() != _fourcc("stbl"):
            return 0
        if not self._container(stbl, "stbl"):
            return 0
        remaining -= stbl
        if remaining != 0:
            self.s.Skip(remaining)
        return 1

    def _stsd(self):  # :412-523
        self.s.Skip(4)
        if self.s.ReadUint32() != 1:
            return 0
        entry_size = self.s.ReadUint32()
        self.res.Format = self.s.ReadUint32()
        remaining = entry_size - 8
        if self.res.Format != _fourcc("alac"):
            return 0
        self.s.Skip(6)
        self.s.ReadUint16()   # version
        self.s.ReadUint16()   # revision
        self.s.ReadUint32()   # vendor
        self.s.ReadUint16()   # the extra 16 bits
        self.s.Skip(4)        # channels, bits per sample (top level)
        self.s.ReadUint16()   # compression id
        self.s.ReadUint16()   # packet size
        self.s.Skip(4)        # sample rate (top level)
        remaining -= 6 + 2 + 6 + 2 + 4 + 4 + 4
        self.res.CodecDataLength = remaining + 12 + 8
        if self.res.CodecDataLength > len(self.res.CodecData):
            return 0
        cd = self.res.CodecData
        for i in range(self.res.CodecDataLength):
            cd[i] = 0
        cd[0], cd[1], cd[2] = 0x0C000000, _fourcc("amrf"), _fourcc("cala")
        payload = self.s.Read(remaining)
        for i, b in enumerate(payload):   # MyStream.Read(int, int[], startPos): one int per byte
            cd[12 + i] = b
        self.res.SampleSize = cd[29] & 0xFF
        self.res.NumChannels = cd[33] & 0xFF
        self.res.SampleRate = ((cd[44] & 0xFF) << 24) | ((cd[45] & 0xFF) << 16) | ((cd[46] & 0xFF) << 8) | (cd[47] & 0xFF)
        self.res.FormatRead = 1
        return 1

    def _stts(self, chunk_len):  # :525-559
        remaining = chunk_len - 8
        self.s.Skip(4)
        n = self.s.ReadUint32()
        remaining -= 8
        if n > 16:
            raise IndexError("Index was outside the bounds of the array.")  # TimeToSample[16], DemuxResT.cs:27
        self.res.NumTimeToSamples = n
        self.res.TimeToSample = []
        for _ in range(n):
            self.res.TimeToSample.append((self.s.ReadUint32(), self.s.ReadUint32()))
            remaining -= 8
        if remaining != 0:
            self.s.Skip(remaining)

    def _stsz(self, chunk_len):  # :561-613
        remaining = chunk_len - 8
        self.s.Skip(4)
        uniform = self.s.ReadUint32()
        if uniform != 0:
            n = self.s.ReadUint32()
            self.res.SampleByteSize = np.full(n, uniform, dtype=np.int64)
            return
        n = self.s.ReadUint32()
        remaining -= 12
        raw = self.s.Read(4 * n)
        self.res.SampleByteSize = np.frombuffer(raw, dtype=">u4").astype(np.int64)
        remaining -= 4 * n
        if remaining != 0:
            self.s.Skip(remaining)

    def _mdat(self, chunk_len, skip):  # :724-734
        remaining = chunk_len - 8
        if remaining == 0:
            return
        self.res.MdatLen = remaining
        if skip:
            self.saved_mdat_pos = self.s.Position
            self.s.Skip(remaining)

    def _set_saved_mdat(self):  # :736-750 (the `!= 0` test makes every non-zero position "cannot seek")
        if self.saved_mdat_pos == -1:
            return MDAT_NO_VALID_SAVED_POS
        if self.s.Seek(self.saved_mdat_pos) != 0:
            return MDAT_CANNOT_SEEK
        return MDAT_OK


def _open_source(source):
    """bytes / bytearray / memoryview, a path, or a seekable binary file object -> (file object, whether to close it)"""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return io.BytesIO(bytes(source)), True
    if isinstance(source, (str, os.PathLike)):
        return open(source, "rb"), True
    return source, False


def _read_headers(f):
    """The movie headers of an open file, read as packet_table reads them: (DemuxResT, the _Stream at the start of the media
    data, durations[n] int64, sizes[n] uint32)."""
    res = DemuxResT()
    stream = _Stream(f)
    head = QtMovieT(stream, res).ReadHeader()
    if head in (MDAT_NONE, MDAT_CANNOT_SEEK):
        raise IOError("Error while loading the QuickTime movie headers.")
    # TryGetSampleInfo (AlacContext.cs:130-156) for every packet: the stts runs, cut where stsz or stts ends
    counts = [int(c) for c, _ in res.TimeToSample[:res.NumTimeToSamples]]
    durs = [int(d) for _, d in res.TimeToSample[:res.NumTimeToSamples]]
    durations = np.repeat(np.array(durs, dtype=np.int64), np.maximum(np.array(counts, dtype=np.int64), 0))
    n = min(len(res.SampleByteSize), len(durations))
    return res, stream, durations[:n].copy(), res.SampleByteSize[:n].astype(np.uint32)


def _stream_facts(res, durations):
    return dict(sample_rate=res.SampleRate if res.SampleRate != 0 else 44100,
                num_channels=res.NumChannels if res.NumChannels != 0 else 2,
                sample_size=res.SampleSize if res.SampleSize != 0 else 16,
                num_samples=int(durations.sum()))


def header_table(source):
    """What the headers of an M4A file say, without its packet bytes (host only, no GPU context): a dict with sizes[n] uint32,
    durations[n] int64 (frames), sample_rate, num_channels, sample_size and num_samples, as packet_table gives them.  ValueError
    for a source that is neither file bytes, a path nor a seekable binary file object."""
    if not isinstance(source, (bytes, bytearray, memoryview, str, os.PathLike)) and \
            not all(hasattr(source, a) for a in ("read", "seek", "tell")):
        raise ValueError(f"source must be file bytes, a path or a seekable binary file object, not {type(source).__name__}")
    f, close = _open_source(source)
    try:
        res, _, durations, sizes = _read_headers(f)
        return dict(sizes=sizes, durations=durations, **_stream_facts(res, durations))
    finally:
        if close:
            f.close()


def packet_table(source):
    """The packet table of an M4A file, on the host only (no GPU context): what alacgpu_decode_into_device needs to place
    every packet of the file in one gap-free tensor.  `source`: file bytes, a path, or a seekable binary file object.
    Packets are taken as AlacContext.ReadBatch takes them: `stsz` sizes, `stts` durations, the bytes read back to back from
    the start of the media data.  Returns a dict:
      sizes[n] uint32, durations[n] int64 (frames), dst_first[n] int64 (exclusive prefix sum of the durations),
      offsets[n] uint64 into blob, blob uint8 (the packet bytes), cfg (one alacgpu_cfg row), sample_rate, num_channels,
      sample_size, num_samples (AlacContext.GetNumSamples: the sum of the durations)."""
    f, close = _open_source(source)
    try:
        res, stream, durations, sizes = _read_headers(f)
        n = len(sizes)
        blob = np.frombuffer(stream.Read(int(sizes.sum(dtype=np.int64))), dtype=np.uint8)
        offsets = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offsets[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
        dst_first = np.zeros(n, dtype=np.int64)
        if n > 1:
            dst_first[1:] = np.cumsum(durations[:-1])
        cfg = cfg_from_codec_data(res.CodecData[:48], res.SampleSize, res.NumChannels)
        return dict(sizes=sizes, durations=durations, dst_first=dst_first, offsets=offsets, blob=blob, cfg=cfg,
                    **_stream_facts(res, durations))
    finally:
        if close:
            f.close()


class AlacContext:
    """Mirror of the reference's public `AlacContext` (AlacContext.cs:20-338) over the GPU decode path."""

    def __init__(self, baseStream, disposeStream=False, device=0, batch_packets=256):
        self._demuxRes = DemuxResT()
        self._stream = _Stream(baseStream)
        self._disposeStream = disposeStream
        head = QtMovieT(self._stream, self._demuxRes).ReadHeader()
        if head in (MDAT_NONE, MDAT_CANNOT_SEEK):
            if disposeStream:
                baseStream.close()
            raise IOError("Error while loading the QuickTime movie headers.")   # AlacContext.cs:50
        self._cfg = cfg_from_codec_data(self._demuxRes.CodecData[:48], self._demuxRes.SampleSize,
                                        self._demuxRes.NumChannels)             # new AlacFile + SetInfo (:54-55)
        self._gpu = AlacGpuContext(self._cfg, device)
        self._batch_packets = max(1, int(batch_packets))
        self._currentSampleBlock = 0
        self._offset = 0
        self.LastSampleNumber = 0
        self._ready = []      # decoded, not yet delivered packets of the current batch: (ref_ints, out_bytes, status)
        self._disposed = False

    # ---- getters (AlacContext.cs:83-101) ----
    def GetSampleRate(self):
        return self._demuxRes.SampleRate if self._demuxRes.SampleRate != 0 else 44100

    def GetNumChannels(self):
        return self._demuxRes.NumChannels if self._demuxRes.NumChannels != 0 else 2

    def GetBitsPerSample(self):
        return self._demuxRes.SampleSize if self._demuxRes.SampleSize != 0 else 16

    def GetBytesPerSample(self):
        return -(-self._demuxRes.SampleSize // 8) if self._demuxRes.SampleSize != 0 else 2

    def _sample_info(self, samplenum):  # TryGetSampleInfo (:130-156) -> (byte size, duration) or None
        r = self._demuxRes
        if samplenum >= len(r.SampleByteSize) or r.NumTimeToSamples == 0:
            return None
        acc = 0
        idx = 0
        while r.TimeToSample[idx][0] + acc <= samplenum:
            acc += r.TimeToSample[idx][0]
            idx += 1
            if idx >= r.NumTimeToSamples:
                return None
        return int(r.SampleByteSize[samplenum]), int(r.TimeToSample[idx][1])

    def GetNumSamples(self):  # :108-122
        total = 0
        for i in range(len(self._demuxRes.SampleByteSize)):
            info = self._sample_info(i)
            if info is None:
                return -1
            total += info[1]
        return total

    # ---- batch entry point (new) ----
    def ReadBatch(self, max_packets=None):
        """Pre-reads up to max_packets packets from the current position and decodes them in one GPU batch.
        Returns (pcm[n_packets, slot] int32, out_samples[n], status[n], durations[n]); advances the cursor."""
        k = self._batch_packets if max_packets is None else max_packets
        sizes, durs = [], []
        blk = self._currentSampleBlock
        while len(sizes) < k:
            info = self._sample_info(blk + len(sizes))
            if info is None:
                break
            sizes.append(info[0])
            durs.append(info[1])
        if not sizes:
            return None
        blob = np.frombuffer(self._stream.Read(int(sum(sizes))), dtype=np.uint8)   # packets are read in file order (:195)
        sizes = np.array(sizes, dtype=np.uint32)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        slot = MAX_FRAME * int(self._cfg[0]["num_channels"])
        slot = min(slot, max(int(self._cfg[0]["max_samples_per_frame"]), 1) * int(self._cfg[0]["num_channels"]) + 8)
        pcm, ob, os_, st = self._gpu.decode_batch(blob, offsets, sizes, None, slot)
        # short frames carry their own sample count; give them room if the stream config under-declares it
        if (st == 4).any():
            slot = MAX_FRAME * int(self._cfg[0]["num_channels"])
            pcm, ob, os_, st = self._gpu.decode_batch(blob, offsets, sizes, None, slot)
        self._currentSampleBlock += len(sizes)
        # a one-channel element with a prediction type other than 0: the reference skips the predictor without throwing and
        # hands out its output buffer, which behind any compressed frame is the residual buffer (AlacFile.cs:484-496 with
        # :486): the library decodes exactly that (status 3 as a warning) -- an ordinary packet from here on
        first = blob[np.minimum(offsets, max(len(blob) - 1, 0)).astype(np.int64)] if len(blob) else np.zeros(len(sizes), np.uint8)
        st = np.where((st == 3) & ((first >> 5) == 0) & (sizes > 0), 0, st).astype(np.int32)
        # a two-channel element in a stream whose sample size is neither 16 / 24 nor 20 / 32: nothing written, no exception (:701-716)
        if int(self._cfg[0]["sample_size"]) not in (16, 24, 20, 32):
            st = np.where((st == 2) & ((first >> 5) == 1) & (sizes > 0), 1, st).astype(np.int32)
        return pcm, ob, os_, st, np.array(durs)

    def Read(self, buffer):
        """int Read(byte[] buffer): one packet per call, little-endian PCM bytes; 0 at end of stream (:163-172)."""
        if not self._ready:
            batch = self.ReadBatch()
            if batch is None:
                return 0
            pcm, ob, os_, st, durs = batch
            for p in range(len(st)):
                self._ready.append((pcm[p], int(ob[p]), int(os_[p]), int(st[p]), int(durs[p])))
        pcm, out_bytes, n, st, dur = self._ready.pop(0)
        if st not in (0, 1):
            _raise_reference_exception(st, self._demuxRes.SampleSize)   # DecodeFrame throws before :198-199 count the packet
        self.LastSampleNumber += dur                              # :199
        ref = expand_reference_layout(self._cfg, pcm, max(n, 0)) if st == 0 else np.zeros(0, dtype=np.int32)
        bps = self.GetBytesPerSample()
        out_bytes -= self._offset * bps                           # :200
        if self._offset:
            ref = ref[self._offset:]                              # Array.Copy(pDest, _offset, pDest, 0, ..) (:201)
        self._offset = 0
        if out_bytes <= 0:
            return max(out_bytes, 0)
        need_ints = out_bytes // 2 if bps == 2 else out_bytes
        if len(ref) < need_ints:
            ref = np.concatenate([ref, np.zeros(need_ints - len(ref), dtype=np.int32)])
        data = format_samples(bps, ref, out_bytes)                # FormatSamples (:168)
        n_out = min(len(data), out_bytes)
        buffer[:n_out] = data[:n_out].tobytes() if isinstance(buffer, (bytearray, memoryview)) else data[:n_out]
        return out_bytes

    def SetPosition(self, position):
        """Sets the position in PCM samples (:262-295), with the reference's chunk/sample walk."""
        r = self._demuxRes
        current_position = 0
        current_sample = 0
        for i, (first_chunk, samples_per_chunk, _) in enumerate(r.Stsc):
            last_chunk = r.Stsc[i + 1][0] if i < len(r.Stsc) - 1 else len(r.Stco)
            for chunk in range(first_chunk, last_chunk + 1):
                if chunk - 1 >= len(r.Stco):
                    raise IndexError("Index was outside the bounds of the array.")
                pos = r.Stco[chunk - 1]
                count = samples_per_chunk
                while count > 0:
                    info = self._sample_info(current_sample)
                    if info is None:
                        break
                    current_position += info[1]
                    if position < current_position:
                        # (only now: a position at or past the end is a no-op in the reference, and Read goes on with the
                        # next packet -- which may be sitting, decoded, in the prefetched batch)
                        self._ready = []
                        self._stream.Seek(pos)
                        self._currentSampleBlock = current_sample
                        self.LastSampleNumber = current_position
                        self._offset = int(position - (current_position - info[1])) * self.GetNumChannels()
                        return
                    pos += info[0]
                    current_sample += 1
                    count -= 1

    def Dispose(self):
        if self._disposed:
            return
        self._gpu.close()
        if self._disposeStream:
            self._stream.f.close()
        self._disposed = True

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.Dispose()


# ---- the writer: packets to an M4A file ---------------------------------------------------------------------------------------
# The atom layout the demuxer above accepts (QTMovieT.cs): ftyp("M4A "), moov{mvhd, trak{tkhd, mdia{mdhd, hdlr, minf{smhd
# (16 bytes), dinf, stbl{stsd{alac}, stts, stsc, stsz, stco}}}}}, mdat -- moov before mdat, one sample description, <= 16 stts
# entries.  alac.net_amd.save writes its files with it; tests and tools make files from synthetic packets with it.
def _atom(name, payload):
    return struct.pack(">I4s", 8 + len(payload), name.encode("ascii")) + payload


def alac_specific_config(frame_len, sample_size, pb, mb, kb, channels, sample_rate, max_frame_bytes=0, avg_bitrate=0):
    """The 24-byte ALACSpecificConfig (what AlacFile.SetInfo parses at CodecData[24..47])."""
    return struct.pack(">IBBBBBBHIII", frame_len, 0, sample_size, pb, mb, kb, channels, 255, max_frame_bytes, avg_bitrate,
                       sample_rate)


def write_m4a(packets, durations, frame_len=4096, sample_size=16, channels=2, sample_rate=44100, pb=40, mb=10, kb=14,
              packets_per_chunk=5, mdat_first=False, uniform_stsz=False, extra_atoms=False, max_frame_bytes=0, avg_bitrate=0):
    """Returns the file as bytes.  durations[i] = PCM frames in packet i.
    max_frame_bytes / avg_bitrate: the cookie's maxFrameBytes and avgBitRate (0: not given).
    uniform_stsz: every packet is zero-padded to the longest one's size and stsz carries that one size (QTMovieT.cs:575-590).
    extra_atoms: adds the atoms the reference skips -- a top-level `free`, `udta` and `free` inside moov, `edts` inside trak
    (QTMovieT.cs:95-102, :135-177, :668-722)."""
    n = len(packets)
    if uniform_stsz:
        size = max(len(p) for p in packets)
        packets = [p + bytes(size - len(p)) for p in packets]
    cfg = alac_specific_config(frame_len, sample_size, pb, mb, kb, channels, sample_rate, max_frame_bytes, avg_bitrate)
    inner = _atom("alac", struct.pack(">I", 0) + cfg)                       # size, 'alac', version/flags, config
    entry = (bytes(6) + struct.pack(">HHIH", 1, 0, 0, 0) + struct.pack(">HH", channels, sample_size)
             + struct.pack(">HH", 0, 0) + struct.pack(">I", sample_rate << 16 & 0xFFFFFFFF) + inner)
    stsd = _atom("stsd", struct.pack(">II", 0, 1) + _atom("alac", entry))
    # stts: run-length of durations (the reference holds at most 16 entries)
    runs = []
    for d in durations:
        if runs and runs[-1][1] == d:
            runs[-1][0] += 1
        else:
            runs.append([1, d])
    assert len(runs) <= 16, "the reference's TimeToSample table has 16 entries"
    stts = _atom("stts", struct.pack(">II", 0, len(runs)) + b"".join(struct.pack(">II", c, d) for c, d in runs))
    if uniform_stsz:
        stsz = _atom("stsz", struct.pack(">III", 0, len(packets[0]), n))
    else:
        stsz = _atom("stsz", struct.pack(">III", 0, 0, n) + b"".join(struct.pack(">I", len(p)) for p in packets))
    n_chunks = (n + packets_per_chunk - 1) // packets_per_chunk
    stsc_entries = [(1, packets_per_chunk, 1)]
    if n % packets_per_chunk and n_chunks > 1:
        stsc_entries.append((n_chunks, n % packets_per_chunk, 1))
    stsc = _atom("stsc", struct.pack(">II", 0, len(stsc_entries)) + b"".join(struct.pack(">III", *e) for e in stsc_entries))

    def build(mdat_offset):
        offs, pos = [], mdat_offset + 8
        for c in range(n_chunks):
            offs.append(pos)
            pos += sum(len(p) for p in packets[c * packets_per_chunk:(c + 1) * packets_per_chunk])
        if offs and offs[-1] >= 1 << 32:
            raise ValueError("the media data lies past the reach of 32-bit chunk offsets (stco)")
        stco = _atom("stco", struct.pack(">II", 0, len(offs)) + b"".join(struct.pack(">I", o) for o in offs))
        stbl = _atom("stbl", stsd + stts + stsc + stsz + stco)
        smhd = _atom("smhd", bytes(8))
        dinf = _atom("dinf", _atom("dref", struct.pack(">II", 0, 1) + _atom("url ", struct.pack(">I", 1))))
        minf = _atom("minf", smhd + dinf + stbl)
        hdlr = _atom("hdlr", struct.pack(">I4s4sIII", 0, b"mhlr", b"soun", 0, 0, 0) + b"\x00")
        mdhd = _atom("mdhd", struct.pack(">IIIIIHH", 0, 0, 0, sample_rate, sum(durations), 0, 0))
        mdia = _atom("mdia", mdhd + hdlr + minf)
        tkhd = _atom("tkhd", bytes(84))
        edts = _atom("edts", _atom("elst", struct.pack(">IIIII", 0, 1, sum(durations), 0, 0x00010000))) if extra_atoms else b""
        trak = _atom("trak", tkhd + edts + mdia)
        mvhd = _atom("mvhd", bytes(100))
        extra = (_atom("udta", _atom("meta", bytes(20))) + _atom("free", bytes(37))) if extra_atoms else b""
        return _atom("moov", mvhd + trak + extra)

    ftyp = _atom("ftyp", b"M4A " + struct.pack(">I", 0) + b"M4A mp42isom")
    if extra_atoms:
        ftyp += _atom("free", bytes(11))
    mdat = _atom("mdat", b"".join(packets))
    if mdat_first:
        moov = build(len(ftyp))
        return ftyp + mdat + moov
    moov = build(0)
    moov = build(len(ftyp) + len(moov))   # offsets depend on moov's (fixed) size
    return ftyp + moov + mdat
