// P/Invoke binding of include/alacgpu.h for the C# host (drop into ALACDecoder/).
// NOT compiled or executed in this repository's pipeline: the build image has no .NET toolchain.
// It is kept mechanical -- blittable arguments only -- and mirrors the executed ctypes binding in
// alac.net_amd/__init__.py (SYMBOLS table) one to one.
using System;
using System.Runtime.InteropServices;

namespace ALACdotNET.Decoder
{
    [StructLayout(LayoutKind.Sequential, Pack = 1, Size = 12)]
    internal struct AlacGpuCfg
    {
        public uint MaxSamplesPerFrame;   // CodecData[24..27]
        public byte SampleSize;           // CodecData[29]
        public byte RiceHistoryMult;      // CodecData[30]
        public byte RiceInitialHistory;   // CodecData[31]
        public byte RiceKModifier;        // CodecData[32]
        public byte NumChannels;          // AlacFile ctor arg
        public byte CtorSampleSize;       // AlacFile ctor arg
        public byte Reserved;
    }

    internal static class AlacGpuNative
    {
        private const string Lib = "alacgpu";   // libalacgpu.so

        public const int StOk = 0, StUnsupportedElement = 1, StUnsupportedSampleSize = 2, StUnsupportedPredType = 3,
                         StBadSampleCount = 4, StOverrun = 5, StRefThrows = 6, StUnsupportedParams = 7, StDestRange = 8;
        public const int OutInt32 = 0, OutPackedLe = 1;
        public const int DstInterleaved = 0, DstPlanar = 1, DstInt32 = 0, DstFloat32 = 1;

        [DllImport(Lib)] public static extern int alacgpu_version();
        [DllImport(Lib)] public static extern int alacgpu_device_count();
        [DllImport(Lib)] public static extern int alacgpu_create([In] AlacGpuCfg[] cfgs, uint nCfgs, int device, out IntPtr ctx);
        [DllImport(Lib)] public static extern void alacgpu_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern int alacgpu_cfg_from_codec_data([In] int[] codecData, uint nInts, int samplesize, int numchannels, out AlacGpuCfg cfg);
        [DllImport(Lib)] public static extern int alacgpu_decode_batch(IntPtr ctx, [In] byte[] blob, ulong blobBytes,
            [In] ulong[] offsets, [In] uint[] sizes, [In] ushort[] cfgIdx, uint nPackets,
            [Out] int[] pcmOut, uint slotInts, [Out] int[] outBytes, [Out] int[] outSamples, [Out] int[] status);
        /// <summary>One batch over several contexts (one per GPU, alacgpu_device_count) from this process: contiguous packet
        /// ranges, one native thread per context, every range writes its own part of the arrays.</summary>
        [DllImport(Lib)] public static extern int alacgpu_decode_batch_sharded([In] IntPtr[] ctxs, uint nCtxs, [In] byte[] blob, ulong blobBytes,
            [In] ulong[] offsets, [In] uint[] sizes, [In] ushort[] cfgIdx, uint nPackets,
            [Out] int[] pcmOut, uint slotInts, [Out] int[] outBytes, [Out] int[] outSamples, [Out] int[] status);
        // the same entry point over raw pointers (pinned / alacgpu_alloc_pinned memory; packed output viewed as bytes)
        [DllImport(Lib, EntryPoint = "alacgpu_decode_batch")] public static extern int alacgpu_decode_batch_ptr(IntPtr ctx, IntPtr blob, ulong blobBytes,
            [In] ulong[] offsets, [In] uint[] sizes, [In] ushort[] cfgIdx, uint nPackets,
            IntPtr pcmOut, uint slotInts, [Out] int[] outBytes, [Out] int[] outSamples, [Out] int[] status);
        /// <summary>Decode into a gap-free int32 / float32 PCM buffer in device memory (every pointer a device pointer,
        /// asynchronous on hipStream); there is no host-buffer variant.</summary>
        [DllImport(Lib)] public static extern int alacgpu_decode_into_device(IntPtr ctx, IntPtr dBlob, ulong blobBytes, IntPtr dOffsets,
            IntPtr dSizes, IntPtr dCfgIdx, uint nPackets, IntPtr dDstFirst, IntPtr dDstFrames, IntPtr dOut, ulong outElems,
            uint channels, int layout, int dtype, ulong planeStride, IntPtr dOutSamples, IntPtr dStatus, IntPtr hipStream);
        /// <summary>Plan nCrops windows of cropFrames frames against a corpus's packet tables in device memory: writes the per-packet
        /// arrays of a window decode (entriesPerCrop entries per crop, padding behind a crop's packets) and dLengths[b]; every
        /// pointer a device pointer, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_plan_crops_device(IntPtr ctx, IntPtr dPktOffset, IntPtr dPktSize, IntPtr dPktEnd,
            IntPtr dFileFirst, IntPtr dFileCfg, uint nFiles, IntPtr dCropFile, IntPtr dCropOffset, uint nCrops, uint cropFrames,
            uint entriesPerCrop, ulong dstStride, IntPtr dOffsets, IntPtr dSizes, IntPtr dCfgIdx, IntPtr dDstFirst, IntPtr dDstFrames,
            IntPtr dSrcSkip, IntPtr dLengths, IntPtr hipStream);
        /// <summary>alacgpu_plan_crops_device with a window length per crop, dCropFrames[b] (uint), cropFrames their bound: a crop
        /// whose length is above it gets dLengths[b] = -1 and no packets.</summary>
        [DllImport(Lib)] public static extern int alacgpu_plan_crops_frames_device(IntPtr ctx, IntPtr dPktOffset, IntPtr dPktSize,
            IntPtr dPktEnd, IntPtr dFileFirst, IntPtr dFileCfg, uint nFiles, IntPtr dCropFile, IntPtr dCropOffset, IntPtr dCropFrames,
            uint nCrops, uint cropFrames, uint entriesPerCrop, ulong dstStride, IntPtr dOffsets, IntPtr dSizes, IntPtr dCfgIdx,
            IntPtr dDstFirst, IntPtr dDstFrames, IntPtr dSrcSkip, IntPtr dLengths, IntPtr hipStream);
        /// <summary>Compact the encoder's packets (packet p in its slot at dPackets + p * slotBytes, its size in dSizes[p]) back to
        /// back into dBlob from byte baseOffset on: writes dPktOffset[p] (ulong) and dTotal[0] (ulong); a packet that would end behind
        /// blobCapacity is not copied.  Every pointer a device pointer, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_compact_packets_device(IntPtr ctx, IntPtr dPackets, ulong slotBytes, IntPtr dSizes,
            uint nPackets, IntPtr dBlob, ulong baseOffset, ulong blobCapacity, IntPtr dPktOffset, IntPtr dTotal, IntPtr hipStream);
        /// <summary>Gather the packets of a plan (dSrcOffset ulong, dSizes uint) out of a corpus whose first loBytes lie at dBlobLo in
        /// device memory and whose other hiBytes at blobHi (device memory or page-locked host memory) into dStage, each at the next
        /// multiple of 16: writes dStageOffset[j] (ulong) and dTotal[0] (ulong); a packet that would end behind stageCapacity is not
        /// copied.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_stage_packets_device(IntPtr ctx, IntPtr dBlobLo, ulong loBytes, IntPtr blobHi,
            ulong hiBytes, IntPtr dSrcOffset, IntPtr dSizes, uint nPackets, IntPtr dStage, ulong stageCapacity, IntPtr dStageOffset,
            IntPtr dTotal, IntPtr hipStream);
        /// <summary>Resample decoded PCM (float32, planar [rows, channels, srcStride]) by the reduced ratio a : b with a polyphase
        /// table (dD0 int[b], dWeights float[b, 2 * width + 1]) into dOut [rows, mono ? 1 : channels, outFrames]; row r holds the
        /// source frames dSrcOrigin[r] .. + dSrcValid[r] (long) of a signal that is zero elsewhere and starts at target frame
        /// dOutFirst[r] (long).  Every pointer a device pointer, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_resample_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, IntPtr dSrcOrigin, IntPtr dSrcValid, IntPtr dOutFirst, ulong outFrames, uint a, uint b, uint width,
            IntPtr dD0, IntPtr dWeights, int mono, IntPtr dOut, IntPtr hipStream);
        /// <summary>One table of alacgpu_resample_rows_device: the ratio a : b, the filter's width, and where the table's d0[b] and
        /// weights[b, 2 * width + 1] start in the call's two arrays (in elements).</summary>
        [StructLayout(LayoutKind.Sequential)] public struct ResampleTable { public uint a, b, width, d0First, weightsFirst; }
        /// <summary>alacgpu_resample_device with a table per row: nTables descriptors (tables on the host, dTables the same on the
        /// device), their d0 and weights one behind the other in dD0 and dWeights, and dRowTable[r] (uint) the table of row r;
        /// a row whose index is nTables or above is written as zeros.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_resample_rows_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, IntPtr dSrcOrigin, IntPtr dSrcValid, IntPtr dOutFirst, ulong outFrames, [In] ResampleTable[] tables,
            IntPtr dTables, uint nTables, IntPtr dD0, IntPtr dWeights, IntPtr dRowTable, int mono, IntPtr dOut, IntPtr hipStream);
        /// <summary>One ratio of alacgpu_resample_ratio_rows_device: a : b and the filter's width; a == 0: the rows that name it
        /// are skipped.</summary>
        [StructLayout(LayoutKind.Sequential)] public struct ResampleRatio { public uint a, b, width; }
        /// <summary>alacgpu_resample_device without tables: nRatios ratios (ratios on the host, dRatios the same on the device) and
        /// dRowRatio[r] (uint) the ratio of row r; every tap's weight is evaluated where it is used.  A row whose index is nRatios
        /// or above, or whose ratio has a == 0, is skipped: its part of dOut stays as it is.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_resample_ratio_rows_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, IntPtr dSrcOrigin, IntPtr dSrcValid, IntPtr dOutFirst, ulong outFrames, [In] ResampleRatio[] ratios,
            IntPtr dRatios, uint nRatios, IntPtr dRowRatio, int mono, IntPtr dOut, IntPtr hipStream);
        /// <summary>Log-mel features of float PCM in device memory (planar [rows, channels, srcStride], the first `frames` of a plane
        /// are signal): frames centred on t * hop with reflection, dWindow [nFft], the DFT against dBasis [nFft, 2 * (nFft / 2 + 1)],
        /// power, dFb [nMels, nFft / 2 + 1], and logMode 0 (none), 1 (ln) or 2 (log10) of max(., floor) into dOut
        /// [rows, channels, nMels, outFrames], outFrames = 1 + frames / hop.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_logmel_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, ulong frames, uint nFft, uint hop, uint nMels, IntPtr dWindow, IntPtr dBasis, IntPtr dFb, int logMode,
            float floor, IntPtr dOut, ulong outFrames, IntPtr hipStream);
        /// <summary>Kaldi's fbank features of float PCM in device memory (planar [rows, channels, srcStride], the first `frames` of a
        /// plane are signal): frames of winLength samples every hop (flags: 1 snip_edges, else centred with Kaldi's reflection), the
        /// frame's mean removed (2), pre-emphasis, dWindow [winLength], the nFft-point DFT against dBasis [winLength,
        /// 2 * (nFft / 2 + 1)], power (4, else magnitude), dFb [nMels, nFft / 2 + 1] and ln(max(., 2^-23)) (8) into dOut
        /// [rows, channels, nMels, outFrames].  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_fbank_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, ulong frames, uint winLength, uint nFft, uint hop, uint nMels, IntPtr dWindow, IntPtr dBasis, IntPtr dFb,
            uint flags, float preemphasis, float scale, IntPtr dOut, ulong outFrames, IntPtr hipStream);
        /// <summary>Kaldi's MFCC features of float PCM in device memory: alacgpu_fbank_device's frames, mean, pre-emphasis, window,
        /// DFT and nMels mel sums (flags 1, 2, 4 as there), then ln(max(., 2^-23)), the projection on dDct [nCeps, nMels] and the
        /// product with dLifter [nCeps] into dOut [rows, channels, nCeps, outFrames]; flags 16 (use_energy): line 0 is the log
        /// energy of the frame (32, raw_energy: before pre-emphasis and window), at least ln(energyFloor) for energyFloor > 0.
        /// Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_mfcc_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, ulong frames, uint winLength, uint nFft, uint hop, uint nMels, uint nCeps, IntPtr dWindow, IntPtr dBasis,
            IntPtr dFb, IntPtr dDct, IntPtr dLifter, uint flags, float preemphasis, float scale, float energyFloor, IntPtr dOut,
            ulong outFrames, IntPtr hipStream);
        /// <summary>Kaldi's add-deltas on float features in device memory (dSrc [rows, channels, nFeats, srcStride], the first lineLen
        /// of a line are frames): the features and their deltas of order 1 .. order (1 .. 3) over window (1 .. 4) frames per order
        /// with the scales dScales, every order clamped into the first min(max(dLengths[row], 0), lineLen) frames of the features
        /// (dLengths: long[rows] or IntPtr.Zero for lineLen), zeros behind them, into dOut [rows, channels, (order + 1) * nFeats,
        /// outStride] apart from dSrc.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_deltas_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows, uint channels,
            uint nFeats, ulong srcStride, ulong outStride, ulong lineLen, IntPtr dLengths, uint order, uint window, IntPtr dScales,
            IntPtr hipStream);
        /// <summary>Mean and variance per line of float data in device memory ([rows, linesPerRow, lineStride], the first lineLen of
        /// a line are data) over the first min(max(dValid[row], 0), lineLen) elements (dValid: long[rows] or IntPtr.Zero for whole
        /// lines): (x - mean) / sqrt(var + eps), zeros behind them, into dOut (dSrc itself or the same layout).  Asynchronous on
        /// hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_normalize_meanvar_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint linesPerRow, ulong lineStride, ulong lineLen, IntPtr dValid, int centre, int scale, float eps, IntPtr hipStream);
        /// <summary>The clamp relative to the maximum mx of a row of the same layout: scale * (max(x, mx - top) [- mx with relative])
        /// + offset into dOut; a row with a NaN is NaN throughout.  Two launches, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_normalize_top_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint linesPerRow, ulong lineStride, ulong lineLen, float top, float scale, float offset, int relative, IntPtr hipStream);
        /// <summary>Kaldi's sliding-window CMVN per line of the same layout over the first min(max(dValid[row], 0), lineLen) frames
        /// (dValid: long[rows] or IntPtr.Zero for whole lines): frame t minus the mean of its window of `window` frames (around it
        /// with center, else behind it and at least minWindow long at the start), divided by the window's standard deviation with
        /// normVars; zeros behind them, into dOut (dSrc itself or the same layout).  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_normalize_sliding_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint linesPerRow, ulong lineStride, ulong lineLen, IntPtr dValid, uint window, uint minWindow, int center, int normVars,
            IntPtr hipStream);
        /// <summary>Per-channel energy normalisation per line of the same layout over the first min(max(dValid[row], 0), lineLen)
        /// frames: s = scale * x, M the first-order smoothing of s with coefficient b from M[0] = s[0], (s / (eps + M)^gain +
        /// bias)^power - biasPow; zeros behind them, into dOut (dSrc itself or the same layout).  biasPow: bias^power.  dTable:
        /// IntPtr.Zero or float[5, linesPerParam] with b, gain, bias, power and bias^power per line % linesPerParam.  stage 1
        /// writes M.  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_pcen_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint linesPerRow, ulong lineStride, ulong lineLen, IntPtr dValid, float b, float gain, float bias, float power,
            float biasPow, float eps, float scale, IntPtr dTable, uint linesPerParam, int stage, IntPtr hipStream);
        /// <summary>Kaldi's energy VAD on the lineLen floats at dSrc + row * rowStride + line of every row, over the first
        /// min(max(dValid[row], 0), lineLen) of them: a frame is voiced (1 in dMask, byte[rows, maskStride]; 0 otherwise and behind
        /// the length) when at least proportionThreshold of the frames within framesContext of it are above energyThreshold +
        /// energyMeanScale * their mean.  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_vad_energy_device(IntPtr ctx, IntPtr dSrc, uint rows, ulong rowStride,
            ulong line, ulong lineLen, IntPtr dValid, float energyThreshold, float energyMeanScale, uint framesContext,
            float proportionThreshold, IntPtr dMask, ulong maskStride, IntPtr hipStream);
        /// <summary>Every line of float data in device memory ([rows, linesPerRow, lineStride]) keeps its frames below
        /// min(max(dValid[row], 0), lineLen) whose dMask[row, t] is not 0, in order, zeros behind them, into dOut (dSrc itself or the
        /// same layout); their number (dValid[row] itself where negative) into dNewLengths (long[rows]; may be dValid).  One launch,
        /// asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_select_frames_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint linesPerRow, ulong lineStride, ulong lineLen, IntPtr dValid, IntPtr dMask, ulong maskStride, IntPtr dNewLengths,
            IntPtr hipStream);
        /// <summary>Noise at a target signal-to-noise ratio into planar float crops in device memory (dSrc, dOut
        /// [rows, channels, stride], dNoise [rows, noiseChannels, noiseStride], noiseChannels 1 or channels; the first frames of a
        /// plane are data): y = x + g n with g = dRatio[row] * sqrt(Ps / Pn) over the first dValid[row] frames of the signal and
        /// dNoiseValid[row] of the noise (long[rows] or IntPtr.Zero for all), the noise repeated where it is the shorter; a ratio
        /// of 0 leaves the row as it is.  dOut is dSrc itself or apart from it.  Two launches, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_mix_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, IntPtr dNoise, uint rows,
            uint channels, uint noiseChannels, ulong stride, ulong noiseStride, ulong frames, IntPtr dValid, IntPtr dNoiseValid,
            IntPtr dRatio, IntPtr hipStream);
        /// <summary>A cascade of biquad sections and a gain per row on planar float crops in device memory (dSrc, dOut
        /// [rows, channels, stride]; the first frames of a plane are data): dCoeffs double[rows, sections, 5] = (b0, b1, b2, a1,
        /// a2), 1 to 8 sections, dGain double[rows] or IntPtr.Zero for 1, over the first dValid[row] frames (long[rows] or
        /// IntPtr.Zero for all), limited to -1 .. 1 with clamp; float64 recurrences, rounded once to float.  A row of identity
        /// sections with gain 1 is left as it is.  dOut is dSrc itself or apart from it.  One launch, asynchronous on
        /// hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_biquad_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint channels, ulong stride, ulong frames, IntPtr dValid, IntPtr dCoeffs, uint sections, IntPtr dGain, int clamp,
            IntPtr hipStream);
        /// <summary>Planar float crops in device memory (dSrc, dOut [rows, channels, stride]; the first frames of a plane are
        /// data) brought to a level over the first dValid[row] frames (long[rows] or IntPtr.Zero for all): mode 0 the peak,
        /// 1 the mean square, 2 the BS.1770-4 integrated loudness with hops of hop frames and the two K-weighting sections
        /// dKweight double[2, 5] (IntPtr.Zero for the other modes).  target is linear (the peak, the mean square,
        /// 10^((LUFS + 0.691) / 10)), maxPeak limits the gain (0: not), clamp limits the result to -1 .. 1.  dGainOut,
        /// dEnergyOut, dPeakOut: double[rows] or IntPtr.Zero.  dOut is dSrc itself, apart from it, or IntPtr.Zero to measure
        /// only.  A row with nothing to measure is left as it is.  Two launches, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_level_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint channels, ulong stride, ulong frames, IntPtr dValid, uint mode, uint hop, IntPtr dKweight, double target,
            double maxPeak, int clamp, IntPtr dGainOut, IntPtr dEnergyOut, IntPtr dPeakOut, IntPtr hipStream);
        /// <summary>The fundamental frequency of planar float crops in device memory (dSrc [rows, channels, stride]; the first
        /// frames of a plane are data), frame by frame: the YIN estimator over the lags tauMin .. tauMax with windows of
        /// winLength samples every hop samples, over the first dValid[row] samples (long[rows] or IntPtr.Zero for all), zeros
        /// outside them; frames centred on t * hop (alignLength 0) or counted and placed as Kaldi's snip_edges frames of
        /// alignLength samples.  dOut is float[rows, channels, 2, outFrames]: f0 in Hz and the aperiodicity, which is below
        /// threshold exactly for a voiced frame; zeros behind a row's frames.  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_yin_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong stride, ulong frames, IntPtr dValid, uint sampleRate, uint winLength, uint hop, uint tauMin, uint tauMax,
            uint alignLength, float threshold, IntPtr dOut, ulong outFrames, IntPtr hipStream);
        /// <summary>The smoothed fundamental frequency of planar float crops in device memory: probabilistic YIN, the troughs of
        /// the YIN estimator's d' with a probability each, then a Viterbi decode over voiced and unvoiced pitch bins along every
        /// plane.  dSrc, dValid and the framing as for alacgpu_yin_device; dTable the specification's packed float tables
        /// (include/alacgpu.h).  stage 0: dOut is float[rows, channels, 3, outFrames] -- the bin's frequency in Hz, 1 where
        /// voiced, the voicing probability; stage 1: the observations alone into dObsVoiced, dObsUnvoiced and dVp; stage 2: the
        /// decode alone on given observations into dStates (int[rows, channels, outFrames]), dValid then counting frames.  Two
        /// launches, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_pyin_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong stride, ulong frames, IntPtr dValid, uint sampleRate, uint winLength, uint hop, uint tauMin, uint tauMax,
            uint alignLength, uint nThresholds, uint nBins, uint band, float noTroughProb, IntPtr dTable, IntPtr dObsVoiced,
            IntPtr dObsUnvoiced, IntPtr dVp, IntPtr dOut, IntPtr dStates, ulong outFrames, int stage, IntPtr hipStream);
        /// <summary>Kaldi's pitch features of planar float crops in device memory (compute-kaldi-pitch-feats and
        /// process-kaldi-pitch-feats): stage 0 everything into dOut [rows, channels, lines, outFrames], 1 the NCCF planes into
        /// dNccf, 2 the decode of dNccf into dRaw, 3 the post-processing of dRaw into dOut; dTable the packed tables of
        /// kaldi_pitch.KaldiPitch.table (include/alacgpu.h).</summary>
        [DllImport(Lib)] public static extern int alacgpu_kaldi_pitch_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong stride, ulong frames, IntPtr dValid, uint sampleRate, uint resampleFreq, uint winLength, uint hop, uint window,
            uint shift, uint firstLag, uint lastLag, uint nStates, uint phases, uint inPerUnit, uint downTaps, uint upTaps,
            uint flags, uint leftContext, uint rightContext, uint deltaWindow, IntPtr dTable, IntPtr dNccf, IntPtr dRaw,
            IntPtr dOut, ulong outFrames, int stage, IntPtr hipStream);
        /// <summary>Constant-Q features of planar float crops in device memory (dSrc [rows, channels, srcStride] to dOut
        /// [rows, channels, nBins, outFrames], outFrames = 1 + frames / hop): lengths is the N_k in host memory, dLengths
        /// the same in device memory, dTable the kernels in blocks of 16 bins (include/alacgpu.h).</summary>
        [DllImport(Lib)] public static extern int alacgpu_cqt_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, ulong frames, uint hop, uint nBins, uint[] lengths, IntPtr dLengths, IntPtr dTable, int power,
            int logMode, float floor, IntPtr dOut, ulong outFrames, IntPtr hipStream);
        /// <summary>Linear, complex or banded (mel) spectrograms of planar float crops in device memory by an FFT (dSrc [rows,
        /// channels, srcStride] to dOut [rows, channels, lines, outFrames], outFrames = 1 + frames / hop): nFft 256, 512, 1024
        /// or 2048; dWindow float[nFft], dTable float[nFft][2]; power 0 the complex spectrum (2 (nFft / 2 + 1) lines), 1
        /// magnitude, 2 power; fbLines 0, or the lines of a filterbank whose bands (first, count, offset per line) are in host
        /// memory, dBands the same in device memory and dWeights the packed weights (include/alacgpu.h).</summary>
        [DllImport(Lib)] public static extern int alacgpu_stft_device(IntPtr ctx, IntPtr dSrc, uint rows, uint channels,
            ulong srcStride, ulong frames, uint nFft, uint hop, IntPtr dWindow, IntPtr dTable, int power, uint fbLines,
            uint[] bands, IntPtr dBands, IntPtr dWeights, int logMode, float floor, IntPtr dOut, ulong outFrames,
            IntPtr hipStream);
        /// <summary>Room reverberation into planar float crops in device memory (dSrc, dOut [rows, channels, stride], dRir
        /// [rows, rirChannels, rirStride], rirChannels 1 or channels; the first frames / rirFrames of a plane are data): every
        /// row convolved with its impulse response over the first dValid[row] frames of the signal and dRirValid[row] of the
        /// response (long[rows] or IntPtr.Zero for all), aligned on the response's largest tap and scaled to unit energy; a
        /// response of 0 valid frames leaves the row as it is.  dOut is dSrc itself or apart from it.  Two launches,
        /// asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_reverb_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, IntPtr dRir, uint rows,
            uint channels, uint rirChannels, ulong stride, ulong rirStride, ulong frames, ulong rirFrames, IntPtr dValid,
            IntPtr dRirValid, IntPtr hipStream);
        /// <summary>Image-source impulse responses of shoebox rooms in device memory (dGeometry double[rows, 9]: room, source
        /// and microphone in metres; dBeta float[rows, 6]: the walls' reflection coefficients; dOut float[rows, outStride] of
        /// which the first frames of a row are written; dLengths int[rows]: frames, or 0 where the row is refused and zeros).
        /// maxOrder -1 takes every reflection order.  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_rir_shoebox_device(IntPtr ctx, IntPtr dGeometry, IntPtr dBeta, uint rows,
            uint sampleRate, ulong frames, uint taps, int maxOrder, double soundSpeed, IntPtr dOut, ulong outStride,
            IntPtr dLengths, IntPtr hipStream);
        /// <summary>Time stretch of planar float crops in device memory with the pitch kept, a phase vocoder (dSrc [rows,
        /// channels, srcStride] of which the first frames are data, dOut [rows, channels, outStride] apart from it, of which
        /// the first outFrames are written): row r is stretched by dP[r] / dQ[r] (int[rows]) over its first dValid[r] frames
        /// (long[rows] or IntPtr.Zero for all) to (2 v p + q) / (2 q) frames, zeros behind them; the new lengths into
        /// dValidOut (long[rows]).  A row with p == q or at most nFft / 2 valid frames is neither read nor written.  nFft: 512,
        /// 1024 or 2048.  Followed by alacgpu_resample_ratio_rows_device at the same ratio it is a pitch shift.  Three
        /// launches, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_time_stretch_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint channels, ulong srcStride, ulong outStride, ulong frames, ulong outFrames, IntPtr dP, IntPtr dQ, IntPtr dValid,
            IntPtr dValidOut, uint nFft, IntPtr hipStream);
        /// <summary>The first dValid[row] frames (long[rows]) of every plane of dSrc [rows, channels, srcStride] copied to dOut
        /// [rows, channels, outStride], apart from it; nothing else is written.  One launch, asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_copy_rows_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint channels, ulong srcStride, ulong outStride, ulong frames, IntPtr dValid, IntPtr hipStream);
        /// <summary>SpecAugment on float features in device memory (dSrc, dOut [rows, channels, nMels, lineStride], the first
        /// lineLen of a line are frames), one launch: per row a time warp (dWarp int[rows, 2]: (c, c'), or IntPtr.Zero for
        /// none), nFreq frequency masks and nTime time masks (dFreq int[rows, nFreq, 2], dTime int[rows, nTime, 2]: (first,
        /// width)) over the first dValid[row] frames (long[rows] or IntPtr.Zero for all), masked elements set to fill.  dOut
        /// is dSrc itself or apart from it.  Asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern int alacgpu_specaugment_device(IntPtr ctx, IntPtr dSrc, IntPtr dOut, uint rows,
            uint channels, uint nMels, ulong lineStride, ulong lineLen, IntPtr dValid, IntPtr dWarp, IntPtr dFreq, uint nFreq,
            IntPtr dTime, uint nTime, float fill, IntPtr hipStream);
        /// <summary>Encode PCM in device memory (int32 or float32, interleaved or planar) to ALAC packets in device memory, one
        /// run of frames per packet, packet p at dPackets + p * slotBytes; asynchronous on hipStream.</summary>
        [DllImport(Lib)] public static extern UIntPtr alacgpu_encode_max_packet_bytes(uint frames, int sampleSize, int channels);
        [DllImport(Lib)] public static extern int alacgpu_encode_device(IntPtr ctx, IntPtr dPcm, ulong srcElems, uint channels, int layout,
            int dtype, ulong planeStride, IntPtr dSrcFirst, IntPtr dSrcFrames, IntPtr dCfgIdx, uint nPackets, IntPtr dPackets,
            ulong slotBytes, IntPtr dSizes, IntPtr dStatus, IntPtr hipStream);
        [DllImport(Lib)] public static extern int alacgpu_decode_frame(IntPtr ctx, uint cfgIndex, [In] byte[] inbuffer, uint inBytes,
            [Out] int[] outbuffer, uint outCapacityInts, out int outBytes, out int status);
        /// <summary>0: one int per sample (default); 1: packed little-endian PCM, the bytes AlacContext.Read returns
        /// (AlacContext.FormatSamples fused into the store) at the start of every slot; out_bytes[p] of them.</summary>
        [DllImport(Lib)] public static extern int alacgpu_set_output_format(IntPtr ctx, int format);
        /// <summary>Pairing (include/alacgpu.h): both channels of a resident packet in one pass, from a remembered and verified start
        /// of channel B; on by default.  Stats: packets decoded paired, without a remembered start, with a wrong one.</summary>
        [DllImport(Lib)] public static extern int alacgpu_set_pairing(IntPtr ctx, int on);
        [DllImport(Lib)] public static extern int alacgpu_pairing_stats(IntPtr ctx, [Out] ulong[] out3);
        [DllImport(Lib)] public static extern int alacgpu_pairing_shift_starts(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr alacgpu_alloc_pinned(UIntPtr bytes);
        [DllImport(Lib)] public static extern void alacgpu_free_pinned(IntPtr p);
        [DllImport(Lib)] public static extern float alacgpu_last_kernel_ms(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr alacgpu_status_string(int status);
        [DllImport(Lib)] public static extern IntPtr alacgpu_strerror(int rc);
        [DllImport(Lib)] public static extern IntPtr alacgpu_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int alacgpu_ctx_device(IntPtr ctx);

        // ---- multi-GPU, one process per GPU: the packet partition and the RCCL all-gather of decoded PCM (include/alacgpu.h) ----
        public const int CommIdBytes = 128;
        /// <summary>first[world + 1]: rank r owns packets first[r] .. first[r+1] (whole groups of 8, balanced by packet bytes).</summary>
        [DllImport(Lib)] public static extern int alacgpu_shard_ranges([In] uint[] sizes, uint nPackets, uint world, [Out] uint[] first);
        /// <summary>Rank 0: 128 bytes to hand to the other ranks (pipe, socket, file ...) before alacgpu_comm_create.</summary>
        [DllImport(Lib)] public static extern int alacgpu_comm_get_unique_id([Out] byte[] id128);
        /// <summary>Collective (ncclCommInitRank): every rank calls it with the same id.</summary>
        [DllImport(Lib)] public static extern int alacgpu_comm_create(IntPtr ctx, [In] byte[] id128, int rank, int world, out IntPtr comm);
        [DllImport(Lib)] public static extern void alacgpu_comm_destroy(IntPtr comm);
        [DllImport(Lib)] public static extern int alacgpu_comm_rank(IntPtr comm);
        [DllImport(Lib)] public static extern int alacgpu_comm_world(IntPtr comm);
        [DllImport(Lib)] public static extern IntPtr alacgpu_comm_last_error(IntPtr comm);
        /// <summary>dFullPcm (device memory, the whole batch's slots in global packet order) holds this rank's packets decoded
        /// in place; on return -- asynchronous on hipStream -- every rank holds every packet (ncclAllGather, int32).</summary>
        [DllImport(Lib)] public static extern int alacgpu_allgather_pcm(IntPtr comm, IntPtr dFullPcm, [In] uint[] first, uint slotInts, IntPtr hipStream);
        /// <summary>Decode this rank's range in up to four pieces and gather piece k while piece k + 1 decodes; all device arrays are
        /// indexed by GLOBAL packet number.</summary>
        [DllImport(Lib)] public static extern int alacgpu_decode_allgather_device(IntPtr ctx, IntPtr comm, IntPtr dBlob, ulong blobBytes,
            IntPtr dOffsets, IntPtr dSizes, IntPtr dCfgIdx, [In] uint[] first, IntPtr dFullPcm, uint slotInts,
            IntPtr dOutBytes, IntPtr dOutSamples, IntPtr dStatus, uint nChunks, IntPtr hipStream);

        public static string Error(int rc) => Marshal.PtrToStringAnsi(alacgpu_strerror(rc));
    }
}
