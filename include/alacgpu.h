/*
 * alacgpu.h -- C ABI of libalacgpu.so: the MI355X (gfx950) batched ALAC frame-decode path.
 *
 * This is the drop-in boundary for teekay/ALAC.NET's per-packet decode seam.  The reference has
 * no FFI; the seam is the managed call
 *     AlacContext.cs:54-55   _alac = new AlacFile(SampleSize, NumChannels); _alac.SetInfo(CodecData);
 *     AlacContext.cs:197     var outputBytes = _alac.DecodeFrame(_readBuffer, pDestBuffer);
 * and each entry point below names the reference member it replaces.  A C# host binds these with
 * [DllImport("alacgpu")].  Plain pointers and sizes only; caller allocates
 * everything; the library never keeps a caller pointer past the call; one ctx per host thread
 * (a ctx is not thread-safe; one thread may keep up to 8 asynchronous device-pointer calls in flight on
 * any streams, see alacgpu_decode_batch_device).  One ctx drives one GPU: a multi-GPU host creates one ctx
 * per device (alacgpu_device_count) -- in this repository one process per GPU (bench.py, sharding.py).
 *
 * Return codes: 0 = the batch ran (inspect status[]), < 0 = batch-level failure.
 * There is NO CPU fallback: if no gfx950 device / kernel image is usable, create fails.
 */
#ifndef ALACGPU_H
#define ALACGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALACGPU_VERSION 3

/* Stream configuration = the AlacFile ctor args + what AlacFile.SetInfo keeps
 * (AlacFile.cs:16-20 and :63-93; CodecData byte offsets in brackets). 12 bytes, blittable. */
typedef struct {
    uint32_t max_samples_per_frame; /* [24..27] BE32, AlacFile.cs:72  */
    uint8_t  sample_size;           /* [29]            AlacFile.cs:76  (16 or 24 decode; others -> status) */
    uint8_t  rice_history_mult;     /* [30]            AlacFile.cs:78  */
    uint8_t  rice_initial_history;  /* [31]            AlacFile.cs:80  */
    uint8_t  rice_kmodifier;        /* [32]            AlacFile.cs:82  (1..255; 0 is refused) */
    uint8_t  num_channels;          /* ctor arg,       AlacFile.cs:18  (1 or 2) */
    uint8_t  ctor_sample_size;      /* ctor arg samplesize (AlacFile.cs:19); 0 = same as sample_size */
    uint8_t  reserved;
} alacgpu_cfg;

/* Per-packet status[] values.  The reference signals these by exceptions / silent no-ops. */
enum {
    ALACGPU_ST_OK = 0,
    ALACGPU_ST_UNSUPPORTED_ELEMENT = 1,     /* channels field not 0/1: reference decodes nothing (AlacFile.cs:437,:577) */
    ALACGPU_ST_UNSUPPORTED_SAMPLE_SIZE = 2, /* Exception("FIXME: unimplemented sample size N") (AlacFile.cs:574,:715) */
    ALACGPU_ST_UNSUPPORTED_PREDTYPE = 3,    /* Exception("FIXME: unhandled predicition type: N") (AlacFile.cs:650,:660) */
    ALACGPU_ST_BAD_SAMPLE_COUNT = 4,        /* hassize count <= 0, > 16384 or > slot (IndexOutOfRangeException) */
    ALACGPU_ST_OVERRUN = 5,                 /* bitstream ran past the packet / zero run past the scratch (AlacFile.cs:242) */
    ALACGPU_ST_REF_THROWS = 6,              /* N == 0 && n > 4096: Array.Copy ArgumentException (AlacFile.cs:264-265) */
    ALACGPU_ST_UNSUPPORTED_PARAMS = 7,      /* header/parameter combination outside the supported domain */
    ALACGPU_ST_DEST_RANGE = 8               /* alacgpu_decode_into_device: the packet's run lies outside the output, or its
                                               stream cfg has another channel count; nothing of it is written */
};

/* Batch-level return codes */
enum {
    ALACGPU_OK = 0,
    ALACGPU_ERR_BAD_ARG = -1,
    ALACGPU_ERR_NO_DEVICE = -2,          /* no usable gfx950 GPU: there is no CPU fallback */
    ALACGPU_ERR_HIP = -3,                /* a HIP runtime call failed; see alacgpu_last_error */
    ALACGPU_ERR_UNSUPPORTED_CONFIG = -4, /* a cfg is outside the kernel's domain (rice_kmodifier 0, channels not 1/2) */
    ALACGPU_ERR_NO_MEMORY = -5,
    ALACGPU_ERR_COMM = -6                /* RCCL could not be loaded or a collective failed; see alacgpu_comm_last_error */
};

typedef struct alacgpu_ctx alacgpu_ctx;

int alacgpu_version(void);

/* Number of usable (gfx950) devices; 0 when there is none (then alacgpu_create fails: no CPU fallback). */
int alacgpu_device_count(void);

/* Replaces `new AlacFile(samplesize, numchannels)` + `SetInfo(codecData)` (AlacContext.cs:54-55)
 * for one or more streams at once (a batch may mix streams through cfg_idx[]).
 * device = HIP device ordinal. */
int alacgpu_create(const alacgpu_cfg* cfgs, uint32_t n_cfgs, int device, alacgpu_ctx** out_ctx);

void alacgpu_destroy(alacgpu_ctx* ctx);

/* Parses the int-per-byte CodecData array exactly as AlacFile.SetInfo does (AlacFile.cs:63-93). */
int alacgpu_cfg_from_codec_data(const int32_t* codec_data_ints, uint32_t n_ints, int samplesize, int numchannels,
                                alacgpu_cfg* out_cfg);

/*
 * Batched AlacFile.DecodeFrame (AlacFile.cs:428-719) on HOST buffers: H2D, decode kernel, D2H; blocking.
 * Batches of 1024 packets and more are cut into two contiguous packet ranges on separate streams so that the
 * upload of one range, the decode of the previous and the download of the one before overlap (needs the packets to
 * lie in the blob in batch order; any other layout works too, with one upload).
 * Bytes outside [offsets[p], offsets[p]+sizes[p]) are never interpreted as part of packet p: a packet that is cut
 * short decodes as if zero bits followed (and reports ALACGPU_ST_OVERRUN).
 *   blob/blob_bytes      concatenated raw ALAC packets
 *   offsets[p], sizes[p] packet p = blob[offsets[p] .. offsets[p]+sizes[p])   (any byte alignment)
 *   cfg_idx[p]           stream cfg of packet p; NULL = all 0
 *   pcm_out              packet p decodes to pcm_out + p*slot_ints, ONE int32 PER SAMPLE interleaved by the
 *                        stream's num_channels (16-bit: exactly the ints DecodeFrame stores; 24-bit: the
 *                        sample sign-extended -- DecodeFrame's byte-per-int layout is alacgpu_expand_reference_layout)
 *   slot_ints            >= max n*num_channels over the batch.  What a slot holds beyond the packet's own output
 *                        (n*num_channels ints, or out_bytes[p] bytes in the packed format) is unspecified: the kernels
 *                        use the slot as scratch while they decode
 *   out_bytes[p]         DecodeFrame's return value (AlacFile.cs:718); may be NULL
 *   out_samples[p]       samples per channel in packet p; may be NULL
 *   status[p]            ALACGPU_ST_*
 */
int alacgpu_decode_batch(alacgpu_ctx* ctx, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offsets,
                         const uint32_t* sizes, const uint16_t* cfg_idx, uint32_t n_packets, int32_t* pcm_out,
                         uint32_t slot_ints, int32_t* out_bytes, int32_t* out_samples, int32_t* status);

/*
 * The same batch over SEVERAL contexts from one process -- normally one context per GPU of the node (alacgpu_device_count,
 * alacgpu_create with device = 0, 1, ...): the packets are cut into n_ctxs contiguous ranges (alacgpu_shard_ranges: whole
 * groups of 8 packets, balanced by packet bytes), one host thread per context runs alacgpu_decode_batch on its range, and
 * every range writes its own part of the caller's arrays (nothing to gather).  All contexts must have been created with
 * the same cfgs and output format and must be DISTINCT (a context is not thread-safe: ALACGPU_ERR_BAD_ARG otherwise).
 * This is how a single-process host (the C# AlacContext) uses every GPU of a node with results in HOST memory; for
 * results that stay in HBM on every GPU see alacgpu_comm_* below (one process per GPU).
 */
int alacgpu_decode_batch_sharded(alacgpu_ctx* const* ctxs, uint32_t n_ctxs, const uint8_t* blob, uint64_t blob_bytes,
                                 const uint64_t* offsets, const uint32_t* sizes, const uint16_t* cfg_idx, uint32_t n_packets,
                                 int32_t* pcm_out, uint32_t slot_ints, int32_t* out_bytes, int32_t* out_samples,
                                 int32_t* status);

/*
 * The packet partition every multi-GPU entry point uses: contiguous ranges, cut at multiples of
 * 8 packets, whose summed packet bytes are as equal as such cuts allow.  first[] gets world + 1 entries; rank r owns
 * packets first[r] .. first[r+1].  Pure host arithmetic (no GPU needed).
 */
int alacgpu_shard_ranges(const uint32_t* sizes, uint32_t n_packets, uint32_t world, uint32_t* first);

/*
 * Multi-GPU, one process per GPU (north_star: "packet batches shard trivially across the 8 GPUs of one node with an RCCL
 * all-gather of decoded PCM over xGMI"; there is no counterpart in the reference, whose AlacContext.cs:195-197 decodes one
 * packet at a time on the host).  Every process makes its alacgpu_ctx, rank 0 makes an id (alacgpu_comm_get_unique_id:
 * 128 bytes) and hands it to the others by whatever channel the host has, and all call alacgpu_comm_create (collective:
 * ncclCommInitRank).  RCCL is loaded when the first of these functions is called (librccl.so, the copy already in the
 * process if there is one); a host that never calls them does not need it.
 *   alacgpu_allgather_pcm          d_full holds the WHOLE batch's slots in global packet order on this rank's GPU; this
 *                                  rank's packets first[rank] .. first[rank+1] are decoded in place; on return (asynchronous
 *                                  on hip_stream) every rank holds every packet: one in-place all-gather(-v) of int32
 *   alacgpu_decode_allgather_device  decode + gather overlapped: this rank's range is decoded in n_chunks (1..4) pieces on
 *                                  hip_stream, piece k is gathered on the communicator's own stream while piece k+1
 *                                  decodes; hip_stream waits for the last gather.  All device arrays are indexed by
 *                                  GLOBAL packet number (the batch's metadata is resident on every GPU).
 * All ranks must make the same calls with the same first[] / n_chunks.  Return codes as elsewhere; ALACGPU_ERR_COMM =
 * RCCL missing or a collective failed (alacgpu_comm_last_error(comm), or (NULL) for the calling thread's last failure).
 */
#define ALACGPU_COMM_ID_BYTES 128
typedef struct alacgpu_comm alacgpu_comm;
int alacgpu_comm_get_unique_id(void* id128);
int alacgpu_comm_create(alacgpu_ctx* ctx, const void* id128, int rank, int world, alacgpu_comm** out_comm);
void alacgpu_comm_destroy(alacgpu_comm* comm);
int alacgpu_comm_rank(const alacgpu_comm* comm);
int alacgpu_comm_world(const alacgpu_comm* comm);
const char* alacgpu_comm_last_error(const alacgpu_comm* comm);
int alacgpu_allgather_pcm(alacgpu_comm* comm, void* d_full_pcm, const uint32_t* first, uint32_t slot_ints, void* hip_stream);
int alacgpu_decode_allgather_device(alacgpu_ctx* ctx, alacgpu_comm* comm, const void* d_blob, uint64_t blob_bytes,
                                    const void* d_offsets, const void* d_sizes, const void* d_cfg_idx, const uint32_t* first,
                                    void* d_full_pcm, uint32_t slot_ints, void* d_out_bytes, void* d_out_samples,
                                    void* d_status, uint32_t n_chunks, void* hip_stream);
/* the device ordinal a context was created on */
int alacgpu_ctx_device(const alacgpu_ctx* ctx);

/*
 * Same, on DEVICE buffers already resident in HBM (all pointers are device pointers), asynchronous on
 * `hip_stream` (a hipStream_t; NULL = default stream).  d_blob must be 16-byte aligned and readable up to
 * blob_bytes rounded up to 16 (ALACGPU_ERR_BAD_ARG otherwise; the other arrays need their natural alignment).
 * Outputs as above; d_out_bytes / d_out_samples may be NULL.  Up to 8 calls may be in flight at once on one ctx, on
 * the same or on different streams (each owns its scratch until it has finished; a ninth call waits for the oldest).
 * The caller keeps every buffer alive and unchanged until the stream has passed the call.
 * Throughput: a launch of a few thousand packets is bound by the length of one packet's serial chain, not by the chip; a
 * caller with a stream of such batches keeps TWO in flight on two streams (0.70 -> about 0.5 ms per batch of 4096 packets,
 * bench.py key two_in_flight; streams that share one of the runtime's hardware queues do not overlap) -- or makes its batches
 * bigger.
 */
int alacgpu_decode_batch_device(alacgpu_ctx* ctx, const void* d_blob, uint64_t blob_bytes, const void* d_offsets,
                                const void* d_sizes, const void* d_cfg_idx, uint32_t n_packets, void* d_pcm_out,
                                uint32_t slot_ints, void* d_out_bytes, void* d_out_samples, void* d_status,
                                void* hip_stream);

/*
 * Decode straight into a gap-free PCM tensor in HBM (no counterpart in the reference, whose AlacContext.Read hands out one
 * packet at a time): the slot layout above, compacted inside the kernels.  Device pointers, asynchronous on hip_stream, up
 * to 8 calls in flight, alignment as for alacgpu_decode_batch_device; d_dst_first is 8-byte aligned, d_out 4-byte aligned.
 *   d_dst_first[p]   uint64: frame index of packet p's first sample
 *   d_dst_frames[p]  uint32: frames reserved for packet p (usually its stts duration)
 *   d_out            out_elems elements of int32 (dtype ALACGPU_DST_INT32: the canonical sample, as the int32 slot format) or
 *                    float32 (ALACGPU_DST_FLOAT32: sample * 2^-(sample_size-1), exact)
 *   layout           ALACGPU_DST_INTERLEAVED: frame i, channel c of packet p at (d_dst_first[p] + i) * channels + c;
 *                    ALACGPU_DST_PLANAR: at c * plane_stride + d_dst_first[p] + i (dst_first = f*C*T + t and plane_stride
 *                    = T address a [F, C, T] tensor)
 *   d_out_samples[p] samples per channel the packet decodes to; may be NULL
 *   d_status[p]      ALACGPU_ST_*: what alacgpu_decode_batch_device reports with slot_ints = channels * Smax (Smax = the
 *                    largest max_samples_per_frame of the ctx's cfgs, at most 16384), or ALACGPU_ST_DEST_RANGE
 * Every element of a packet's run (frames 0 .. d_dst_frames[p] of every channel) is written unless its status is
 * ALACGPU_ST_DEST_RANGE: the decoded frames (those from d_dst_frames[p] on are dropped: a last packet longer than its
 * duration), then zeros.  A packet that fails gets a run of zeros; a one-channel element with an unknown prediction type
 * (status 3) keeps its un-predicted residuals, as in the slot layout; a one-channel element in a two-channel stream has
 * zeros in channel 1.  Elements outside every run are never touched.  Channel A of a two-channel packet waits in scratch
 * the ctx owns (n_packets * Smax ints per call in flight, kept for reuse).  ALACGPU_ERR_BAD_ARG: a NULL ctx or array
 * (d_cfg_idx and d_out_samples may be NULL), channels not 1 / 2, an unknown layout or dtype, planar with plane_stride 0.
 * Host-buffer callers (the C# AlacContext) have no variant of this: they get the slot layout.
 */
enum { ALACGPU_DST_INTERLEAVED = 0, ALACGPU_DST_PLANAR = 1 };
enum { ALACGPU_DST_INT32 = 0, ALACGPU_DST_FLOAT32 = 1 };
int alacgpu_decode_into_device(alacgpu_ctx* ctx, const void* d_blob, uint64_t blob_bytes, const void* d_offsets,
                               const void* d_sizes, const void* d_cfg_idx, uint32_t n_packets,
                               const void* d_dst_first, const void* d_dst_frames, void* d_out, uint64_t out_elems,
                               uint32_t channels, int layout, int dtype, uint64_t plane_stride,
                               void* d_out_samples, void* d_status, void* hip_stream);

/*
 * A window of every packet (no counterpart in the reference): alacgpu_decode_into_device, with packet p's run starting
 * d_src_skip[p] frames into the packet -- what a crop of a file at any frame offset needs for the packet it starts in.
 *   d_src_skip[p]    uint32, 4-byte aligned: frames i with d_src_skip[p] <= i < d_src_skip[p] + d_dst_frames[p] form the run;
 *                    frame i, channel c goes to frame d_dst_first[p] + (i - d_src_skip[p]) in either layout.  A skip above
 *                    16384 (the longest frame) is status ALACGPU_ST_DEST_RANGE.  NULL: no skip -- exactly
 *                    alacgpu_decode_into_device, which is this entry point with NULL.
 * Every element of a packet's run is written unless its status is ALACGPU_ST_DEST_RANGE: the decoded frames of the window, then
 * zeros (for the window's frames past the packet's decoded ones); a packet that fails gets a run of zeros.  Statuses and
 * d_out_samples[p] are those of alacgpu_decode_into_device (but for a skip above 16384): the whole packet is decoded, the
 * skip only chooses what is stored.  With a skip array the ctx keeps n_packets uint64 more scratch per call in flight (kept for
 * reuse).  ALACGPU_ERR_BAD_ARG as for alacgpu_decode_into_device, and for a misaligned d_src_skip.
 */
int alacgpu_decode_window_into_device(alacgpu_ctx* ctx, const void* d_blob, uint64_t blob_bytes, const void* d_offsets,
                                      const void* d_sizes, const void* d_cfg_idx, uint32_t n_packets,
                                      const void* d_dst_first, const void* d_dst_frames, const void* d_src_skip,
                                      void* d_out, uint64_t out_elems, uint32_t channels, int layout, int dtype,
                                      uint64_t plane_stride, void* d_out_samples, void* d_status, void* hip_stream);

/*
 * Plan the crops of a corpus that is resident in HBM (no counterpart in the reference): for n_crops windows of crop_frames
 * frames each, crop b = (file d_crop_file[b], first frame d_crop_offset[b]), write the per-packet arrays that
 * alacgpu_decode_window_into_device reads -- one more call decodes every crop, and the host never sees the plan.  Device
 * pointers only (natural alignment), asynchronous on hip_stream; nothing of the ctx is used but its device.
 * The resident tables, built once per corpus (P packets of F files, the files' packets back to back):
 *   d_pkt_offset[P]   uint64: byte offset of the packet into the resident blob
 *   d_pkt_size[P]     uint32: its size (stsz)
 *   d_pkt_end[P]      uint64: the frames of the packet's FILE up to and including this packet (inclusive prefix sum of the
 *                     stts durations, starting anew with every file); T_f, a file's frame count, is its last packet's value
 *   d_file_first[F+1] uint32: the first packet of file f; file f's packets are d_file_first[f] .. d_file_first[f+1]
 *   d_file_cfg[F]     uint16: the file's stream cfg (a row of the decoding ctx)
 * The call: d_crop_file[b] uint32, d_crop_offset[b] uint64, and entries_per_crop (K): the entries reserved per crop.
 * The plan, n_crops * K entries, crop b's at j = b * K + i: d_offsets[j] uint64, d_sizes[j] uint32, d_cfg_idx[j] uint16,
 * d_dst_first[j] uint64 = b * dst_stride + the run's first frame in the crop (dst_stride = C * crop_frames addresses a
 * planar [B, C, crop_frames] tensor), d_dst_frames[j] uint32, d_src_skip[j] uint32 (at most 16384: frames further into a
 * packet are zeros); and d_lengths[b] int64:
 *   min(crop_frames, T_f - offset)   the crop's frames; its entries are the packets that overlap frames offset .. offset +
 *                                    length of the file, in file order (a crop from frame 0 starts at packet 0; packets
 *                                    without frames are taken only between others; a crop of length 0 has no packets)
 *   -1                               d_crop_file[b] >= n_files or offset > T_f: no packets
 *   -2                               the crop needs more than K entries: no packets
 * The entries behind a crop's packets are padding: cfg_idx 0xFFFF and zeros.  In a decode call such an entry has status
 * ALACGPU_ST_UNSUPPORTED_PARAMS, costs no decode step and writes nothing (a ctx has at most 65535 cfgs for that).  Nothing
 * outside the n_crops * K entries and the n_crops lengths is ever written.  n_crops == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG: a NULL ctx or array, a misaligned array, K == 0, or n_crops * K above 2^32 - 1.  The tables are the
 * caller's: d_file_first ascending with d_file_first[F] <= P, d_pkt_end ascending within a file.
 */
int alacgpu_plan_crops_device(alacgpu_ctx* ctx, const void* d_pkt_offset, const void* d_pkt_size, const void* d_pkt_end,
                              const void* d_file_first, const void* d_file_cfg, uint32_t n_files,
                              const void* d_crop_file, const void* d_crop_offset, uint32_t n_crops,
                              uint32_t crop_frames, uint32_t entries_per_crop, uint64_t dst_stride,
                              void* d_offsets, void* d_sizes, void* d_cfg_idx, void* d_dst_first, void* d_dst_frames,
                              void* d_src_skip, void* d_lengths, void* hip_stream);

/*
 * alacgpu_plan_crops_device with a window length per crop (no counterpart in the reference): the crops of files of different
 * sample rates need different numbers of source frames for the same frames at the target rate.  Everything is as above but
 *   d_crop_frames[b]  uint32: crop b's window length; crop_frames is the bound of them all and dst_stride stays the uniform
 *                     row stride (C * crop_frames addresses a planar [B, C, crop_frames] tensor)
 *   d_lengths[b]      min(d_crop_frames[b], T_f - offset); -1 also for a d_crop_frames[b] above crop_frames: no packets, so
 *                     nothing is ever planned outside a row; -2 as above
 * With every d_crop_frames[b] equal to crop_frames the plan is the one alacgpu_plan_crops_device writes, bit for bit.
 * ALACGPU_ERR_BAD_ARG as above, and for a NULL or misaligned (4) d_crop_frames.
 */
int alacgpu_plan_crops_frames_device(alacgpu_ctx* ctx, const void* d_pkt_offset, const void* d_pkt_size, const void* d_pkt_end,
                                     const void* d_file_first, const void* d_file_cfg, uint32_t n_files,
                                     const void* d_crop_file, const void* d_crop_offset, const void* d_crop_frames,
                                     uint32_t n_crops, uint32_t crop_frames, uint32_t entries_per_crop, uint64_t dst_stride,
                                     void* d_offsets, void* d_sizes, void* d_cfg_idx, void* d_dst_first, void* d_dst_frames,
                                     void* d_src_skip, void* d_lengths, void* hip_stream);

/*
 * Encoder (no counterpart in the reference, which only decodes): PCM in HBM to ALAC packets in HBM, one packet per run of
 * frames, asynchronous on hip_stream.  Device pointers; d_pcm 4-byte, d_src_first 8-byte, d_packets 16-byte aligned.
 *   d_pcm            src_elems int32 (ALACGPU_DST_INT32: the canonical sample, clamped to the sample range) or float32
 *                    (ALACGPU_DST_FLOAT32: round(x * 2^(sample_size-1)), clamped) elements, laid out as for
 *                    alacgpu_decode_into_device: frame t, channel c at t * channels + c or c * plane_stride + t
 *   d_src_first[p]   uint64: first frame of packet p;  d_src_frames[p] uint32: its frame count (1 .. the cfg's
 *                    max_samples_per_frame, at most 16384)
 *   d_cfg_idx[p]     uint16: the stream cfg of packet p (ctx->cfgs); it gives sample_size (16 or 24), pb / mb / kb and
 *                    max_samples_per_frame (hassize is set exactly when a packet is shorter)
 *   d_packets        packet p is written at d_packets + p * slot_bytes; slot_bytes is a multiple of 16 and at least
 *                    alacgpu_encode_max_packet_bytes(max_samples_per_frame, sample_size, channels) for every cfg
 *   d_sizes[p]       uint32: packet p's size in bytes (0 when it failed)
 *   d_status[p]      ALACGPU_ST_OK; ALACGPU_ST_BAD_SAMPLE_COUNT (0 frames or more than the cfg allows),
 *                    ALACGPU_ST_DEST_RANGE (the run lies outside the source), ALACGPU_ST_UNSUPPORTED_SAMPLE_SIZE,
 *                    ALACGPU_ST_UNSUPPORTED_PARAMS (cfg index out of range): such a packet's slot is not touched
 * The encoder's fixed policy (alac_encode.hip): 16-bit without and 24-bit with one uncompressed low byte; a two-channel
 * stream tries mix shift 2 with weights 0..4; LPC order 8 at q = 9, predictionType 0, ricemodifier 4; an escape packet when
 * the compressed one would not be smaller, so no packet exceeds alacgpu_encode_max_packet_bytes.  The packet bytes past
 * d_sizes[p] up to the next multiple of 4 are zero; the rest of the slot is not touched.  The ctx keeps a workspace
 * (36 bytes per frame of max_samples_per_frame for each of up to 16 packets per CU); calls on one ctx run one after the other
 * on the device.  ALACGPU_ERR_BAD_ARG: a NULL ctx or array, channels not those of every cfg of the ctx, an unknown layout or
 * dtype, planar with plane_stride 0, a misaligned pointer, or a slot_bytes below the bound.
 */
size_t alacgpu_encode_max_packet_bytes(uint32_t frames, int sample_size, int channels);
int alacgpu_encode_device(alacgpu_ctx* ctx, const void* d_pcm, uint64_t src_elems, uint32_t channels, int layout, int dtype,
                          uint64_t plane_stride, const void* d_src_first, const void* d_src_frames, const void* d_cfg_idx,
                          uint32_t n_packets, void* d_packets, uint64_t slot_bytes, void* d_sizes, void* d_status,
                          void* hip_stream);

/*
 * Compact the encoder's packets into the resident layout of a corpus (no counterpart in the reference): from packet p in its
 * own slot at d_packets + p * slot_bytes (what alacgpu_encode_device leaves behind) to the packets back to back, byte
 * granular, in d_blob from byte `base` on, plus the offsets the decoder and alacgpu_plan_crops_device read.  Device pointers,
 * asynchronous on hip_stream; the library reads nothing back.
 *   d_packets        16-byte aligned, slot_bytes a multiple of 16;  d_sizes[p] uint32: packet p's size.  A size above
 *                    slot_bytes counts as 0: whatever the device data say, nothing outside a slot is read
 *   d_pkt_offset[p]  uint64, written: base + the counted sizes of the packets q < p (base of any alignment: a second batch
 *                    lands right behind the first; base + the total must fit 64 bits)
 *   d_total[0]       uint64, written: the sum of the counted sizes
 *   d_blob           any alignment.  Packet p is copied to d_blob + d_pkt_offset[p] iff d_pkt_offset[p] + its size <=
 *                    blob_capacity; a packet that does not fit is not copied at all (the caller sees base + total >
 *                    blob_capacity, grows the blob and calls again).  No byte of d_blob outside the copied packets is
 *                    written.  d_pkt_offset and d_total are written in full either way.
 * n_packets == 0: d_total[0] = 0 and nothing else.  The ctx keeps the scan's partial sums (8 bytes per 2048 packets); calls
 * on one ctx run one after the other on the device.  The scan is a hierarchy of launches (no workgroup waits for another);
 * the copy is spread over the destination's bytes, so many small packets cost what few large ones do.
 * ALACGPU_ERR_BAD_ARG: a NULL ctx or array, slot_bytes 0 or not a multiple of 16, a misaligned d_packets (16), d_sizes (4),
 * d_pkt_offset (8) or d_total (8).
 */
int alacgpu_compact_packets_device(alacgpu_ctx* ctx, const void* d_packets, uint64_t slot_bytes, const void* d_sizes,
                                   uint32_t n_packets, void* d_blob, uint64_t base, uint64_t blob_capacity,
                                   void* d_pkt_offset, void* d_total, void* hip_stream);

/*
 * Stage the packets of a plan (no counterpart in the reference): gather them out of a corpus that lies partly in device memory
 * and partly in page-locked host memory into one small blob in device memory, every packet at the next multiple of 16.  It
 * sits between alacgpu_plan_crops_device and alacgpu_decode_window_into_device, which then reads d_stage with d_stage_offset
 * as its offsets and stage_capacity as its blob_bytes; the decode kernels never read host memory themselves.  Asynchronous on
 * hip_stream; the library reads nothing back.
 *   the source       one address space: offset x < lo_bytes is byte x of d_blob_lo (device memory), every other one byte
 *                    x - lo_bytes of blob_hi.  Either part may be NULL with 0 bytes.  blob_hi is a device pointer or
 *                    page-locked host memory (alacgpu_alloc_pinned, hipHostMalloc, hipHostRegister): the library takes its
 *                    device view.  Both bases 16-byte aligned and readable up to their size rounded up to 16
 *   d_src_offset[j]  uint64, d_sizes[j] uint32: packet j of the plan (a plan's offsets and sizes, padding entries included).
 *                    A packet counts with its size when it lies wholly inside one of the two parts; one that reaches past
 *                    the end of the space or straddles lo_bytes counts as 0: whatever the device data say, nothing outside
 *                    the two parts' rounded-up extents is read.  Size 0 copies nothing
 *   d_stage_offset[j] uint64, written in full: the sum over q < j of the counted sizes each rounded up to 16
 *   d_total[0]       uint64, written: that sum over all packets, whatever the capacity
 *   d_stage          16-byte aligned.  Packet j is copied to d_stage + d_stage_offset[j] iff d_stage_offset[j] + its size
 *                    rounded up to 16 <= stage_capacity, otherwise not at all.  No byte at or behind min(total,
 *                    stage_capacity) is written; the bytes between a packet's end and its round-up are unspecified
 * n_packets == 0: d_total[0] = 0 and nothing else.  The scan is the compaction's (a hierarchy of launches, no workgroup waits
 * for another) and shares the ctx's partial sums with it: calls on one ctx run one after the other on the device.  The copy
 * is spread over the staging blob's 16-byte chunks, each one packet's and one store; it is shaped for the link: a lane has up
 * to sixteen independent 16-byte loads in flight before its first store, a source that is not aligned as its destination is
 * read as two aligned chunks, and no source byte is fetched by more than the two lanes that share a chunk edge.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a NULL base with non-zero bytes, a misaligned base
 * or d_stage (16), d_sizes (4), d_src_offset, d_stage_offset or d_total (8), a blob_hi that is neither device memory nor
 * page-locked.
 */
int alacgpu_stage_packets_device(alacgpu_ctx* ctx, const void* d_blob_lo, uint64_t lo_bytes, const void* blob_hi, uint64_t hi_bytes,
                                 const void* d_src_offset, const void* d_sizes, uint32_t n_packets, void* d_stage,
                                 uint64_t stage_capacity, void* d_stage_offset, void* d_total, void* hip_stream);

/*
 * Resample decoded PCM to another rate (no counterpart in the reference): a polyphase Hann-windowed sinc behind the decode.
 * a : b is the reduced ratio source rate : target rate.  The filter is the caller's table (alac.net_amd/resample.py builds the
 * one this library documents: rolloff 0.99, 6 zero crossings): target frame j = i + b * m is
 *   y[j] = sum over n < N of d_weights[i * N + n] * x[m * a + d_d0[i] + n],   N = 2 * width + 1,
 * in float32 with one fused multiply-add per tap in ascending n.  d_d0[i] (int32, [b]) is floor(i * a / b) - width for every
 * table that call builds; the kernel relies on d_d0 ascending with i and on d_d0[i] + N <= d_d0[0] + a + 2 * width + 1.
 * Device pointers only, asynchronous on hip_stream, nothing is read back; nothing of the ctx is used but its device.
 *   d_src            float32, planar [rows, channels, src_stride]; channels 1 or 2
 *   d_src_origin[r]  int64: the absolute source frame of element 0 of row r
 *   d_src_valid[r]   int64: the frames behind it that hold signal (clamped to 0 .. src_stride).  x is zero at every frame
 *                    outside [origin, origin + valid), negative frames included, whatever the memory holds: nothing outside
 *                    that range is read
 *   d_out_first[r]   int64: the absolute target frame of output element 0 of row r
 *   d_out            float32 [rows, mono ? 1 : channels, out_frames]; every element is written.  The resampled signal of row r
 *                    has ceil(b * (origin + valid) / a) frames; an output frame outside 0 .. that count is written as zero
 *   mono             non-zero: two channels become one, (x[0] + x[1]) * 0.5 in float32 in front of the filter; with one
 *                    channel it changes nothing
 * A whole signal is origin 0, first 0, valid its length and out_frames ceil(b * valid / a).  b * (origin + valid) and
 * (first + out_frames) * a must fit 63 bits.  A workgroup holds the table and the source span of a tile of output frames in
 * LDS (up to 160 KiB for ratios in the hundreds; 64 KiB and less for audio rates).  rows == 0 or out_frames == 0: nothing
 * happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a misaligned array (8 for the three int64 arrays, 4
 * for the others), a, b or width 0, b * (2 * width + 1) above 16384, channels not 1 or 2, 2^31 tiles of output or more (a tile
 * is 1024 frames of one row and channel for audio rates).
 */
int alacgpu_resample_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                            const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
                            uint32_t a, uint32_t b, uint32_t width, const void* d_d0, const void* d_weights, int mono,
                            void* d_out, void* hip_stream);

/*
 * alacgpu_resample_device with a table per row (no counterpart in the reference): the rows of one call are crops of files of
 * different sample rates, all resampled to one target rate.  The call has n_tables tables; table t is a : b and width as
 * above, its d0[b] starts at element d0_first of d_d0 and its weights[b, 2 * width + 1] at element weights_first of d_weights.
 *   tables, d_tables  the n_tables descriptors twice: in host memory, where the call checks them and sizes the launch, and in
 *                     device memory (4-byte aligned), where the kernel reads them.  They must agree; a workgroup that reads a
 *                     descriptor that does not fit the launch writes its row as zeros, so nothing outside d_out or the
 *                     workgroup's LDS is ever stored to.  Nothing is read back
 *   d_row_table[r]    uint32: the table of row r.  A row with d_row_table[r] >= n_tables is written as zeros (the row of a
 *                     crop outside the corpus)
 * Everything else -- d_src, d_src_origin, d_src_valid, d_out_first, d_out, mono -- is alacgpu_resample_device's, and row r is
 * what that call computes for the row with row r's table: the same float32 fused multiply-adds in the same order, so the two
 * agree bit for bit.  One tile (output frames per workgroup step) serves the whole launch, chosen as above for the table that
 * needs the most LDS for it; a workgroup loads its own row's table and uses its own table's span.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: as above, and n_tables == 0, a NULL or misaligned `tables`, d_tables or
 * d_row_table, or any table with a, b or width 0 or b * (2 * width + 1) above 16384.
 */
typedef struct alacgpu_resample_table {
    uint32_t a, b, width;
    uint32_t d0_first;
    uint32_t weights_first;
} alacgpu_resample_table;
int alacgpu_resample_rows_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                                 const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
                                 const alacgpu_resample_table* tables, const void* d_tables, uint32_t n_tables,
                                 const void* d_d0, const void* d_weights, const void* d_row_table, int mono, void* d_out,
                                 void* hip_stream);

/*
 * The resampler without tables (no counterpart in the reference): a ratio per row, and every tap's weight evaluated where it is
 * used -- what speed perturbation needs, whose ratios (44.1 kHz played at 0.9 to 16 kHz is 3969 : 1600, 52800 weights) no table
 * in LDS holds.  Row r with the ratio a : b and width computes what alacgpu_resample_device defines,
 *   y[j] = sum over d = -width .. width of w(d b - (j a mod b)) * x[floor(j a / b) + d],
 *   w(n) = scale * sinc(v) * cos^2(pi v / 12) for |v| < 6, else 0,   v = 99 n / (100 max(a, b)),   scale = 0.99 min(a, b) / a,
 * with j a mod b and floor(j a / b) in 64-bit integers.  A weight is evaluated in float32 from the integer 99 n, reduced modulo
 * the period of the sine before anything is rounded, by a polynomial of degree 13 for each of sin(pi v) and cos(pi v / 12), one
 * correctly rounded division and four products (alac.net_amd/speed.py states every operation, and its numpy twin restates it: no
 * hardware approximation is used); it is within 2^-18 * scale of the weight above.  The taps are accumulated by fused
 * multiply-adds in ascending d, as the table kernels do.
 *   ratios, d_ratios  the n_ratios ratios twice: in host memory, where the call checks them and sizes the launch, and in device
 *                     memory (4-byte aligned), where the kernel reads them.  They must agree; a workgroup that reads a ratio
 *                     that does not fit the launch skips its row.  width: the filter's reach in source frames, at least
 *                     600 a / (99 min(a, b)) for the whole filter (resample.filter_width); taps outside |v| < 6 weigh nothing
 *   d_row_ratio[r]    uint32: the ratio of row r.  A row with d_row_ratio[r] >= n_ratios, or whose ratio has a == 0, is SKIPPED:
 *                     its part of d_out is left as it is (rows another call has written or will write)
 * Everything else -- d_src, d_src_origin, d_src_valid, d_out_first, d_out, mono -- is alacgpu_resample_device's; every element
 * of a row that is not skipped is written, by one writer.  One tile serves the whole launch, chosen as above for the ratio whose
 * span of it is the longest; the LDS holds that span only.  The largest ratio: a frame's own span, 2 width + 2 floats, has to
 * fit 160 KiB, so width <= 20479 and a / b up to about 3378 (48 kHz at factor 1.1 to 8 kHz is 33 : 5).
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: as alacgpu_resample_device for what it shares, and n_ratios == 0, a NULL or
 * misaligned `ratios`, d_ratios or d_row_ratio, any ratio with b == 0 or with a or b at or above 2^31, any ratio with a != 0 and
 * width 0 or above 20479.
 */
typedef struct alacgpu_resample_ratio {
    uint32_t a, b, width;
} alacgpu_resample_ratio;
int alacgpu_resample_ratio_rows_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                                       const void* d_src_origin, const void* d_src_valid, const void* d_out_first,
                                       uint64_t out_frames, const alacgpu_resample_ratio* ratios, const void* d_ratios,
                                       uint32_t n_ratios, const void* d_row_ratio, int mono, void* d_out, void* hip_stream);

/*
 * Log-mel features of decoded PCM (no counterpart in the reference): framing, window, DFT, power, mel projection and log in
 * one launch.  For every plane (row, channel) x[0 .. frames) and every frame t of 0 .. out_frames, out_frames =
 * 1 + frames / hop, centred on sample t * hop:
 *   x_t[n]   = x[t * hop - n_fft / 2 + n], n < n_fft, reflected once at either end (index -i reads x[i], index
 *              frames - 1 + i reads x[frames - 1 - i]; what one reflection does not bring inside 0 .. frames -- only an odd
 *              n_fft at frames = n_fft / 2 + 1 -- counts as zero)
 *   X[j]     = sum over n of (d_window[n] * x_t[n]) * d_basis[n * 2 * n_bins + j],   j < 2 * n_bins, n_bins = n_fft / 2 + 1
 *   P[k]     = X[k]^2 + X[n_bins + k]^2
 *   M[m]     = sum over k of d_fb[m * n_bins + k] * P[k]
 *   out[m,t] = M[m] (log_mode 0), ln(max(M[m], floor)) (1) or log10(max(M[m], floor)) (2)
 * in float32: one rounding of the window product, then fused multiply-adds in ascending n and k (the DFT on the exact-f32
 * matrix instruction).  The three tables are the caller's (alac.net_amd/features.py builds the ones this library documents: a
 * periodic Hann window, the real DFT's cosines and negated sines, a Slaney or HTK mel filterbank), so any window, basis or
 * filterbank of those shapes is honoured.  Device pointers only, asynchronous on hip_stream, nothing is read back; nothing of
 * the ctx is used but its device.
 *   d_src     float32, planar [rows, channels, src_stride]; only the first `frames` elements of a plane are signal and only
 *             they are read
 *   d_window  float32 [n_fft];  d_basis  float32 [n_fft, 2 * n_bins];  d_fb  float32 [n_mels, n_bins]
 *   d_out     float32 [rows, channels, n_mels, out_frames]; every element is written, each by one thread
 * A workgroup takes 32 consecutive frames of one plane (fewer where 31 * hop + n_fft is above 19456 samples) and holds their
 * span of signal in LDS, 61 KiB in all at n_fft 400, hop 160 and 80 mels and at most 153 KiB.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a misaligned array (4), n_fft outside 16 .. 2048, hop
 * outside 1 .. n_fft, n_mels outside 1 .. 256, a floor that is not positive and finite, a log_mode other than 0, 1, 2,
 * channels 0, frames <= n_fft / 2 or above src_stride, out_frames != 1 + frames / hop, 2^31 workgroups or more.
 */
int alacgpu_logmel_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                          uint64_t frames, uint32_t n_fft, uint32_t hop, uint32_t n_mels, const void* d_window,
                          const void* d_basis, const void* d_fb, int log_mode, float floor, void* d_out,
                          uint64_t out_frames, void* hip_stream);

/*
 * Kaldi filterbank features of decoded PCM (no counterpart in the reference): what Kaldi's compute-fbank-feats computes, in one
 * launch.  For every plane (row, channel) x[0 .. frames) and every frame t of 0 .. out_frames, with N = win_length and
 * n_bins = n_fft / 2 + 1:
 *   flags & 1 (snip_edges)   out_frames = 0 for frames < N, else 1 + (frames - N) / hop; frame t starts at g0 = t * hop
 *   otherwise                out_frames = (frames + hop / 2) / hop; g0 = t * hop + hop / 2 - N / 2, and an index g outside
 *                            0 .. frames is reflected as Kaldi does: m = g mod 2 frames (floored), then m if m < frames, else
 *                            2 frames - 1 - m
 *   s[n]     = scale * x[g0 + n],  n < N
 *   d[n]     = s[n] - (sum of s) / N                       (flags & 2, remove_dc_offset; else d = s)
 *   y[n]     = d[n] - preemphasis * d[n - 1], d[-1] = d[0]  (preemphasis != 0; else y = d)
 *   X[j]     = sum over n of (d_window[n] * y[n]) * d_basis[n * 2 * n_bins + j],   j < 2 * n_bins
 *   P[k]     = X[k]^2 + X[n_bins + k]^2                     (flags & 4, use_power; else its square root)
 *   M[m]     = sum over k of d_fb[m * n_bins + k] * P[k]
 *   out[m,t] = ln(max(M[m], 2^-23)) (flags & 8, log) or M[m]
 * in float32, every operation rounded once: the sum of a frame as eight partial sums (partial j over the taps j, j + 8 ... in
 * ascending order) added as ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), the division and the root correctly rounded, y one
 * fused multiply-add, then fused multiply-adds in ascending n and k (the DFT on the exact-f32 matrix instruction).  The three
 * tables are the caller's (alac.net_amd/fbank.py builds Kaldi's: the Povey window and its kin, the cosines and negated sines
 * of the n_fft-point transform for the N taps that are not padding, mel banks linear on the mel axis), so any window, basis or
 * filterbank of those shapes is honoured.  Device pointers only, asynchronous on hip_stream, nothing is read back; nothing of
 * the ctx is used but its device.
 *   d_src     float32, planar [rows, channels, src_stride]; only the first `frames` elements of a plane are signal and only
 *             they are read
 *   d_window  float32 [N];  d_basis  float32 [N, 2 * n_bins];  d_fb  float32 [n_mels, n_bins]
 *   d_out     float32 [rows, channels, n_mels, out_frames]; every element is written, each by one thread
 * A workgroup takes 32 consecutive frames of one plane (fewer where 31 * hop + N is above 19456 samples) and holds their span of
 * signal in LDS.  rows == 0 or out_frames == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a misaligned array (4), win_length outside 16 .. 2048,
 * n_fft outside win_length .. 2048, hop outside 1 .. win_length, n_mels outside 1 .. 256, flags above 15, a preemphasis outside
 * 0 .. 1, a scale that is zero or not finite, channels 0, frames 0 or above src_stride, out_frames other than the count above,
 * 2^31 workgroups or more.
 */
int alacgpu_fbank_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                         uint64_t frames, uint32_t win_length, uint32_t n_fft, uint32_t hop, uint32_t n_mels,
                         const void* d_window, const void* d_basis, const void* d_fb, uint32_t flags, float preemphasis,
                         float scale, void* d_out, uint64_t out_frames, void* hip_stream);

/*
 * Kaldi MFCC features of decoded PCM (no counterpart in the reference): what Kaldi's compute-mfcc-feats computes, in one
 * launch.  Frames, s, d, y, X, P and M are alacgpu_fbank_device's, by the same flags 1 (snip_edges), 2 (remove_dc_offset) and
 * 4 (use_power) and in the same float32 order; the log is not a choice (flag 8 is refused).  Then per frame, c < n_ceps:
 *   lm[m]    = ln(max(M[m], 2^-23))
 *   C[c]     = sum over m of d_dct[c * n_mels + m] * lm[m]      (fused multiply-adds in ascending m from zero)
 *   out[c,t] = d_lifter[c] * C[c]                               (one product)
 *   E        = ln(max(sum over n of e[n]^2, 2^-23))             (flags & 16, use_energy.  flags & 32, raw_energy: e = d, the
 *                                                                frame after scale and mean, before pre-emphasis and window;
 *                                                                else e = d_window[n] * y[n])
 *   E        = max(E, ln(energy_floor))                         (energy_floor > 0; its log is taken once, in double, and rounded)
 *   out[0,t] = E                                                (use_energy: in the place of C[0], un-liftered)
 * The sum of the squares follows the mean: eight partial sums, partial j over the taps j, j + 8 ... in ascending order, each a
 * chain part = fma(e, e, part), added as ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  The five tables are the caller's
 * (alac.net_amd/mfcc.py builds Kaldi's: fbank's three, the orthonormal DCT-II and the lifter 1 + Q / 2 sin(pi c / Q)).  Device
 * pointers only, asynchronous on hip_stream, nothing is read back; nothing of the ctx is used but its device.
 *   d_src     float32, planar [rows, channels, src_stride]; only the first `frames` elements of a plane are signal and only
 *             they are read
 *   d_window  float32 [N];  d_basis  float32 [N, 2 * n_bins];  d_fb  float32 [n_mels, n_bins]
 *   d_dct     float32 [n_ceps, n_mels];  d_lifter  float32 [n_ceps]
 *   d_out     float32 [rows, channels, n_ceps, out_frames]; every element is written, each by one thread
 * A workgroup is alacgpu_fbank_device's, with 32 more floats of LDS for the energies; the projection runs on the mel sums
 * where they are.  rows == 0 or out_frames == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: what alacgpu_fbank_device refuses, n_ceps outside 1 .. n_mels, a NULL or
 * misaligned d_dct or d_lifter, flags outside 1, 2, 4, 16, 32, flag 32 without 16, an energy_floor that is negative or not
 * finite.
 */
int alacgpu_mfcc_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                        uint64_t frames, uint32_t win_length, uint32_t n_fft, uint32_t hop, uint32_t n_mels, uint32_t n_ceps,
                        const void* d_window, const void* d_basis, const void* d_fb, const void* d_dct, const void* d_lifter,
                        uint32_t flags, float preemphasis, float scale, float energy_floor, void* d_out, uint64_t out_frames,
                        void* hip_stream);

/*
 * Kaldi's add-deltas behind the features (no counterpart in the reference): the features and their time derivatives up to
 * `order`, in one launch.  d_src is float32 [rows, channels, n_feats, src_stride], d_out float32 [rows, channels,
 * (order + 1) * n_feats, out_stride]; the first line_len elements of a line are frames, what lies behind them is neither
 * read nor written.  With W = window, len = min(max(d_lengths[row], 0), line_len) (line_len for a NULL d_lengths) and the
 * scales of order k, 2 k W + 1 of them, at d_scales + W k (k - 1) + (k - 1):
 *   out[f, t]               = x[f, t]                                                          every t < line_len
 *   out[k * n_feats + f, t] = sum over j = -k W .. k W of scales_k[j + k W] * x[f, clamp(t + j, 0, len - 1)]    t < len
 *                           = 0                                                                len <= t < line_len
 * one chain of float32 fused multiply-adds in ascending j from zero.  The clamp is into x for every order, as in Kaldi's
 * DeltaFeatures (alac.net_amd/deltas.py builds its scales: scales_k = scales_{k-1} convolved with [-W .. W] / (2 sum of j^2));
 * any table of that length is honoured.  For a delta nothing at or behind len is read.  Device pointers only, asynchronous on
 * hip_stream, nothing is read back; nothing of the ctx is used but its device.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out or d_scales, a misaligned array (4; d_lengths 8),
 * channels, n_feats or line_len 0, channels * n_feats * 4 above 2^32 - 1, line_len above a stride, order outside 1 .. 3, window
 * outside 1 .. 4, d_src and d_out that overlap, 2^31 workgroups or more.
 */
int alacgpu_deltas_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint32_t n_feats,
                          uint64_t src_stride, uint64_t out_stride, uint64_t line_len, const void* d_lengths, uint32_t order,
                          uint32_t window, const void* d_scales, void* hip_stream);

/*
 * The two normalisations between crops or their features and a model (no counterpart in the reference).  The data of both is
 * float32 [rows, lines_per_row, line_stride]: the first line_len <= line_stride elements of a line are data, what lies behind
 * them is neither read nor written.  Features [B, C, n_mels, Tf] are rows = B, lines_per_row = C * n_mels; a waveform
 * [B, C, T] is rows = B, lines_per_row = C.  d_out is d_src itself (in place) or an array of the same layout apart from it.
 * Device pointers only, asynchronous on hip_stream, nothing is read back.  rows == 0: nothing happens.
 *
 * alacgpu_normalize_meanvar_device: mean and variance per line over the valid elements, one launch.  For line l of row r,
 * v = min(max(d_valid[r], 0), line_len) (d_valid: int64 [rows]; NULL: v = line_len) and
 *   mean = (sum of x[0 .. v)) / v
 *   var  = (sum of (x[i] - mean)^2) / v                      two passes, never E[x^2] - mean^2
 *   y[i] = (x[i] - mean) / sqrt(var + eps)    for i < v      (x[i] - mean with scale 0; x[i] / sqrt(var + eps) with centre 0)
 *   y[i] = 0                                  for v <= i < line_len
 * v = 0 (d_valid[r] = -1 included) writes a line of zeros and reads nothing.  Every operation is one IEEE float32 operation,
 * the divisions and the root correctly rounded, no multiply fused into an add.  The sums are float32 in a fixed order: with
 * P = 64 for line_len <= 256 and P = 1024 above, partial j is ((0 + t[j]) + t[j + P]) + t[j + 2 P] ... in ascending index
 * below v; each run of 64 partials is added as a tree of halves (q[j] += q[j + h], h = 32 .. 1) and the 16 sums of those
 * runs by the same tree (h = 8 .. 1).  A constant line with eps = 0 is 0 / 0 = NaN; a NaN or an infinity inside 0 .. v
 * reaches its own line and no other, one at or behind v nothing.  Lines of up to 256 elements are taken by a wave each, four
 * to a workgroup, and held in registers between the passes; longer ones by a workgroup of 1024 threads each, held in LDS up
 * to 8192 elements and read again from memory (the L2) above.  Nothing of the ctx is used but its device.
 *
 * alacgpu_normalize_top_device: the clamp relative to the maximum of a row, two launches, no atomics.  With mx the maximum
 * of all lines_per_row * line_len elements of the row,
 *   c = mx - top;  z = max(x, c);  z = z - mx (only with relative != 0);  y = (scale * z) + offset
 * each operation rounded once to float32, the product and the sum apart.  A maximum keeps a NaN as np.max does: a row with a
 * NaN anywhere is NaN everywhere, every other row is untouched by it; mx = +inf follows IEEE (c = +inf, and inf - inf with
 * relative).  The result is therefore specified bit for bit, but for the sign of a zero.  Whisper's input is log10 mel power
 * with top 8, scale 0.25, offset 1; decibels with a top_db of 80 are top 8, scale 10, offset 0 on log10 power.  The first
 * launch writes the maximum of every part of a row -- 4096 consecutive elements, or the smallest multiple of 4096 that keeps
 * a row within 1024 parts -- into the ctx's scratch [rows, parts], the second combines a row's parts and writes the result;
 * both are grids of rows * parts workgroups.  Calls of one ctx share that scratch one after the other, whatever their
 * streams (as alacgpu_compact_packets_device's do).
 *
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_out, a misaligned array (4; 8 for d_valid),
 * lines_per_row 0, line_len 0 or above line_stride, d_src and d_out that overlap without being equal, an extent of 2^60
 * bytes or more, 2^31 workgroups or more; eps negative or not finite, centre and scale both 0; top negative or not finite,
 * scale or offset not finite.
 */
int alacgpu_normalize_meanvar_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                     uint64_t line_stride, uint64_t line_len, const void* d_valid, int centre, int scale,
                                     float eps, void* hip_stream);
int alacgpu_normalize_top_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                 uint64_t line_stride, uint64_t line_len, float top, float scale, float offset, int relative,
                                 void* hip_stream);

/*
 * alacgpu_normalize_sliding_device: Kaldi's sliding-window mean (and variance) normalisation behind the features
 * (apply-cmvn-sliding; no counterpart in the reference), one launch.  The layout and the in-place rule are
 * alacgpu_normalize_meanvar_device's: float32 [rows, lines_per_row, line_stride], the first line_len of a line are frames, d_out
 * is d_src itself or an array of that layout apart from it.  Neither Kaldi nor torchaudio is at hand where this is built: the
 * parity is with this specification, SlidingWindowCmnInternal restated.  For line l of row r, v = min(max(d_valid[r], 0),
 * line_len) (d_valid: int64 [rows]; NULL: v = line_len), and for frame t < v the window [s, e), Kaldi's with its quirks (the
 * non-centred window behind frame `window` is window + 1 frames long):
 *   center:      s = t - window / 2;  e = s + window            otherwise:   s = t - window;  e = t + 1
 *   if s < 0:                 e -= s;  s = 0
 *   if not center and e > t:  e = max(t + 1, min_window)
 *   if e > v:                 s -= e - v;  e = v;  s = max(s, 0)
 *   N = e - s;  m = (sum of x[s .. e)) / N
 *   y[t] = x[t] - m                                                                  norm_vars 0
 *   y[t] = N == 1 ? 0 : (x[t] - m) / sqrt(max((sum of x[s .. e)^2) / N - m^2, 1e-10))     norm_vars != 0
 *   y[t] = 0                                                                         for v <= t < line_len
 * v = 0 (d_valid[r] = -1 included) writes a line of zeros and reads nothing.  The float32 arithmetic, one IEEE operation at a
 * time, nothing contracted, divisions and the root correctly rounded: the pivot p = fl(P / fl(v)), P the sum over [0, v) in
 * alacgpu_normalize_meanvar_device's order (64 partial sums for line_len <= 256, 1024 above) of the elements that are finite
 * (another counts as +0); d[t] = fl(x[t] - p), and everything else works on d, so the variance is never E[x^2] - m^2 on data with
 * an offset.  Frames are in blocks of 32 from the line's start; a block's sum is a tree of halves (q[j] += q[j + h], h = 16 .. 1)
 * over its elements, those at or behind v counting as +0, and the same over fl(d * d) with norm_vars.  A window's sums S1 (of d)
 * and S2 (of fl(d * d)) are each one chain of additions from zero: with j0 = ceil(s / 32) and j1 = floor(e / 32) the elements
 * s .. 32 j0 - 1, the blocks j0 .. j1 - 1, the elements 32 j1 .. e - 1, each ascending; all elements ascending where j0 >= j1.
 * A window sum is never a difference of running sums: its error depends on N, not on t or line_len.  m = fl(S1 / fl(N)),
 * y = fl(d[t] - m); with norm_vars var = fl(fl(S2 / fl(N)) - fl(m * m)), floored at 1e-10f (a NaN stays one), and
 * y = fl(fl(d[t] - m) / sqrt(var)).  alac.net_amd/sliding.py derives the error bound.  A NaN or an infinity at t0 < v reaches
 * exactly the frames whose window holds t0, one at or behind v nothing.  Lines of up to 256 frames are taken by a wave each,
 * four to a workgroup; longer ones by a workgroup of 1024 threads each.  d and the block sums are held in LDS, the whole line up
 * to 16384 frames (68 KiB: two workgroups fit the 160 KiB of a CU); a longer line goes through the same LDS as a ring, read a
 * second time from memory in front of the chunk of 1024 frames that needs it and always before the chunk that writes it, which
 * takes a window of at most 7648 frames.  Nothing of the ctx is used but its device, there is no ctx scratch: calls on
 * different streams are independent.  Device pointers only, asynchronous on hip_stream, nothing is read back.  rows == 0: nothing
 * happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_out, a misaligned array (4; 8 for d_valid),
 * lines_per_row 0, line_len 0 or above line_stride, d_src and d_out that overlap without being equal, an extent of 2^60 bytes
 * or more, 2^31 workgroups or more; window or min_window 0 or above 2^31 - 1, min_window above window; a window above 7648 with
 * a line_len above 16384.
 */
int alacgpu_normalize_sliding_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                     uint64_t line_stride, uint64_t line_len, const void* d_valid, uint32_t window,
                                     uint32_t min_window, int center, int norm_vars, void* hip_stream);

/*
 * alacgpu_pcen_device: per-channel energy normalisation of mel or constant-Q energies (Wang et al. 2017, librosa.pcen; no
 * counterpart in the reference), one launch.  The layout and the in-place rule are alacgpu_normalize_meanvar_device's: float32
 * [rows, lines_per_row, line_stride], the first line_len of a line are frames, d_out is d_src itself or an array of that layout
 * apart from it.  For line l of row r, v = min(max(d_valid[r], 0), line_len) (d_valid: int64 [rows]; NULL: v = line_len):
 *   s[t] = scale * x[t]
 *   M[0] = s[0];  M[t] = (1 - b) M[t - 1] + b s[t]                            0 < t < v
 *   y[t] = (s[t] / (eps + M[t])^gain + bias)^power - bias^power                 t < v
 *   y[t] = 0                                                                    v <= t < line_len
 * M[0] = s[0] is the steady state librosa.pcen starts from.  stage 1 writes M instead of y.  bias_pow is bias^power, computed in
 * float64 and rounded once by the caller.  d_table: NULL, and b, gain, bias, power and bias_pow hold for every line; or float32
 * [5, lines_per_param] -- the rows b, gain, bias, power, bias^power --, and line l takes column l % lines_per_param (the
 * per-bin values of a trained front end; lines_per_param divides lines_per_row), the five scalars are then ignored.
 * The float32 arithmetic, one IEEE operation at a time, nothing contracted: the smoother is a blocked scan -- a lane takes 4
 * consecutive frames, a wave scans its 64 affine maps (A, B), A = a^k by repeated multiplication, with __shfl_up, a carry goes
 * from a pass to the next -- in the order csrc/alac_pcen.h states, and x^gain and w^power are exp2(gain log2 x) from two explicit
 * polynomials of that header, so that alac.net_amd/pcen.py's twin is the kernel bit for bit; that module derives the error bound.
 * A NaN or an infinity at t0 < v reaches the frames t0 .. v - 1 of its own line, one at or behind v nothing; v = 0 (d_valid[r] =
 * -1 included) writes a line of zeros and reads nothing.  Lines of up to 1024 frames are taken by a wave each, four to a
 * workgroup; longer ones by a workgroup of 256 threads each; no line length is refused.  Nothing of the ctx is used but its
 * device, there is no ctx scratch and no atomic: calls on different streams are independent.  Device pointers only,
 * asynchronous on hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_out, a misaligned array (4; 8 for d_valid),
 * lines_per_row 0, line_len 0 or above line_stride, d_src and d_out that overlap without being equal, an extent of 2^60 bytes
 * or more, 2^31 workgroups or more; a stage other than 0 and 1; eps or scale not above 0 or not finite; without d_table: b outside
 * (0, 1], gain, bias or bias_pow below 0, power not above 0, any of them not finite; with d_table: lines_per_param 0 or not a
 * divisor of lines_per_row.
 */
int alacgpu_pcen_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                        uint64_t line_stride, uint64_t line_len, const void* d_valid, float b, float gain, float bias, float power,
                        float bias_pow, float eps, float scale, const void* d_table, uint32_t lines_per_param, int stage,
                        void* hip_stream);

/*
 * The energy VAD of the Kaldi speaker recipes on one feature line (compute-vad-decision) and the selection of the voiced
 * frames (select-voiced-frames); no counterpart in the reference, one launch each.  The parity is with this specification,
 * Kaldi's ComputeVadEnergy restated.  Both: device pointers only, asynchronous on hip_stream, nothing is read back, nothing of
 * the ctx is used but its device and there is no ctx scratch, so calls on different streams are independent.  rows == 0:
 * nothing happens.
 *
 * alacgpu_vad_energy_device: E, the energy line of row r, is the line_len floats at d_src + r * row_stride + line (for features
 * [B, C, lines, S]: row_stride = C * lines * S, line = the feature's index * S: the first channel's).  With v =
 * min(max(d_valid[r], 0), line_len) (int64 [rows]; NULL: line_len) and c = frames_context,
 *   thr     = energy_threshold + energy_mean_scale * (sum of E[0 .. v)) / v      (energy_threshold itself with a scale of 0)
 *   num[t]  = #{t2 in [t - c, t + c] and [0, v) : E[t2] > thr},   den[t] = #{t2 in [t - c, t + c] and [0, v)}
 *   d_mask[r * mask_stride + t] = num[t] >= den[t] * proportion_threshold ? 1 : 0   for t < v;   0 for v <= t < line_len
 * in float32: the sum in alacgpu_normalize_meanvar_device's order (64 partial sums for line_len <= 256, 1024 above), mean =
 * fl(sum / fl(v)), thr = fl(energy_threshold + fl(energy_mean_scale * mean)), nothing contracted; the counts are integers and
 * the last comparison is float(num) >= fl(float(den) * proportion_threshold).  A NaN energy compares false; with a scale of 0
 * the mean is not computed.  d_mask is uint8 [rows, mask_stride]: every t < line_len of a row is written, what lies behind is
 * neither read nor written.  A wave per row of up to 256 frames, four to a workgroup, a workgroup of 1024 threads above.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_mask, a misaligned array (4; 8 for d_valid; 1 for
 * d_mask), line_len 0 or above mask_stride, line + line_len above row_stride, a threshold or the scale not finite, a negative
 * scale, frames_context above 64, proportion_threshold outside 0 .. 1, a d_mask that overlaps d_src, an extent of 2^60 bytes or
 * more, 2^31 workgroups or more.
 *
 * alacgpu_select_frames_device: the layout and the in-place rule of alacgpu_normalize_meanvar_device.  For every line of row r,
 * with t_k the k-th t < v whose d_mask[r * mask_stride + t] != 0 and K their number,
 *   y[k] = x[t_k]   for k < K;      y[k] = 0   for K <= k < line_len;      d_new_lengths[r] = d_valid[r] < 0 ? d_valid[r] : K
 * bits are moved, nothing is computed.  What lies behind line_len is neither read nor written.  In place is safe because a
 * frame only moves left: a workgroup of 1024 threads walks its lines in chunks of 1024 frames in ascending order -- a chunk is
 * read, then a barrier, then it is stored -- with the mask's running count carried from chunk to chunk.  A workgroup takes
 * 8 lines of a row; d_new_lengths (int64 [rows]) may be d_valid itself, and then one workgroup takes all lines of a row, since
 * no other may read the length it writes.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out, d_mask or d_new_lengths, a misaligned array (4;
 * 8 for d_valid and d_new_lengths; 1 for d_mask), lines_per_row 0, line_len 0 or above line_stride or mask_stride, d_src and
 * d_out that overlap without being equal, a d_mask or d_new_lengths that overlaps d_src, d_out or one another, a d_new_lengths
 * that overlaps d_valid without being equal, an extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_vad_energy_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint64_t row_stride, uint64_t line,
                              uint64_t line_len, const void* d_valid, float energy_threshold, float energy_mean_scale,
                              uint32_t frames_context, float proportion_threshold, void* d_mask, uint64_t mask_stride,
                              void* hip_stream);
int alacgpu_select_frames_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                 uint64_t line_stride, uint64_t line_len, const void* d_valid, const void* d_mask,
                                 uint64_t mask_stride, void* d_new_lengths, void* hip_stream);

/*
 * alacgpu_mix_device: noise at a target signal-to-noise ratio into the crops, in front of the features (no counterpart in the
 * reference); two launches, no atomics.  The layout is planar float32: d_src and d_out [rows, channels, stride], d_noise
 * [rows, noise_channels, noise_stride] with noise_channels 1 (the one channel goes into every channel of the signal) or
 * channels; the first `frames` elements of a plane are data, what lies behind them is neither read nor written.  d_out is
 * d_src itself (in place) or an array of that layout apart from it.  For row r, with v = min(max(d_valid[r], 0), frames),
 * vn = min(max(d_noise_valid[r], 0), frames) (int64 [rows]; NULL: frames) and a = d_ratio[r] (float32 [rows]; the amplitude
 * ratio 10^(-snr_db / 20), computed by the caller: a power of ten is not correctly rounded and is not this kernel's),
 *   Ps = (sum over c, i < v  of x[c, i]^2) / fl(channels * v)
 *   Pn = (sum over c, i < vn of n[c, i]^2) / fl(noise_channels * vn)       over the noise's own frames, not the repeated ones
 *   g  = a * sqrt(Ps / Pn)                                                 but g = 0 where a == 0, v == 0, vn == 0 or Pn == 0
 *   y[c, i] = x[c, i] + g * n[c mod noise_channels, i mod vn]   for i < v      noise shorter than the crop is repeated
 *   y[c, i] = x[c, i]                                           for v <= i < frames (in place: untouched)
 * Where g == 0 the row's noise is not read by the second launch and y is x bit for bit (in place: nothing is written); a row
 * with a == 0, v == 0 or vn == 0 reads no noise at all, so "no noise for this crop" is a ratio of 0 and a silent noise clip
 * cannot make a NaN.  Every operation is one IEEE float32 operation, the divisions and the root correctly rounded, no multiply
 * fused into an add; the counts are converted with one rounding.  Anything else follows IEEE: a negative, infinite or NaN
 * ratio is data; a NaN or an infinity in x below v, or in n below vn of a row with a != 0, reaches that row and no other; one
 * at or behind v (vn) is never read; Ps == 0 gives g = 0 by the formula.  The sums are float32 in a fixed order: a row is cut
 * into parts of 4096 frames (the smallest multiple of 4096 that keeps a row within 256 parts); within a part partial j of
 * 1024 takes the squares of the frames j, j + 1024, ... of the part, channel after channel, in ascending order; the 4
 * partials of a thread, the 64 sums of a wave and the 4 of a workgroup are each added as a tree of halves (q[j] += q[j + h],
 * h = 2, 1; 32 .. 1; 2, 1), and the parts of a row in ascending order.  The first launch writes both sums of every part into
 * the ctx's scratch [rows, parts, 2], the second combines a row's parts, computes g and writes its part of y; both are grids
 * of rows * parts workgroups, with 16-byte loads and stores where an array's base and stride are multiples of 16 bytes.
 * Calls of one ctx share that scratch one after the other, whatever their streams (as alacgpu_normalize_top_device's do).
 * Device pointers only, asynchronous on hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out, d_noise or d_ratio, a misaligned array (4; 8 for
 * d_valid and d_noise_valid), channels 0, noise_channels neither 1 nor channels, frames 0 or above either stride, d_src and
 * d_out that overlap without being equal, d_noise overlapping d_out, an extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_mix_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, const void* d_noise, uint32_t rows, uint32_t channels,
                       uint32_t noise_channels, uint64_t stride, uint64_t noise_stride, uint64_t frames,
                       const void* d_valid, const void* d_noise_valid, const void* d_ratio, void* hip_stream);

/*
 * alacgpu_biquad_device: a cascade of second-order IIR sections and a gain per row on the crops, behind the noise mix and in
 * front of the features (no counterpart in the reference): volume perturbation, band-limiting, random EQ; one launch, no
 * atomics, no scratch, the same inputs give the same bits.  The layout is planar float32: d_src and d_out [rows, channels,
 * stride], the first `frames` elements of a plane are data, what lies behind them is neither read nor written.  d_out is d_src
 * itself (in place) or an array of that layout apart from it.  For row r, with v = min(max(d_valid[r], 0), frames) (int64
 * [rows]; NULL: frames), q = d_coeffs[r] (float64 [rows, sections, 5] = (b0, b1, b2, a1, a2), a0 divided out, 1 <= sections
 * <= 8) and g = d_gain[r] (float64 [rows]; NULL: 1), u_0 = x widened to float64, every section from zero history,
 *   u_{k+1}[n] = b0 u_k[n] + b1 u_k[n-1] + b2 u_k[n-2] - a1 u_{k+1}[n-1] - a2 u_{k+1}[n-2]     for n < v, in float64
 *   y[c, n]    = fl32(g * u_sections[n])                           rounded once; with clamp then min(max(y, -1), 1), a NaN kept
 * Frames at or behind v are untouched (out of place too: d_out keeps what it held), and a row whose sections are all exactly
 * (1, 0, 0, 0, 0) with a gain of exactly 1 and no clamp is neither read nor written: "nothing for this crop".  The recurrence
 * is evaluated blocked, not sample after sample: a workgroup of 256 lanes takes a (row, channel) in tiles of 4096 frames in
 * ascending order, a lane 16 consecutive frames in registers as float64 through all sections, nothing rounded between them;
 * per section the FIR part and the zero-state recursion over the chunk, the chunk-end states combined by a scan with the
 * powers of the section's 2 x 2 transition matrix (6 steps within a wave, then wave after wave, the last state carried to the
 * next tile), and the incoming state added through the section's two homogeneous responses, which are run once per row and
 * section.  Every operation is one IEEE float64 operation in a fixed order, none fused (csrc/alac_biquad.h and
 * alac.net_amd/biquad.py state it; the twin there equals the kernel bit for bit, and the module derives how far the blocked
 * evaluation may be from the sequential one).  Anything else follows IEEE: coefficients and gains that are not finite, and
 * poles outside the unit circle, are data; a NaN in x below v reaches later frames of its own plane only; one at or behind v
 * is never read.  Loads and stores are 16 bytes wide where both bases and the stride are multiples of 16 bytes, single frames
 * otherwise, with the same result.  A tile is read before it is written and nothing behind it is read again.  Nothing of the
 * ctx is used but its device, so calls on different streams are independent.  Device pointers only, asynchronous on
 * hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out or d_coeffs, a misaligned array (4; 8 for d_valid,
 * d_coeffs and d_gain), channels 0, sections 0 or above 8, frames 0 or above stride, d_src and d_out that overlap without
 * being equal, d_coeffs or d_gain overlapping d_out, an extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_biquad_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t stride,
                          uint64_t frames, const void* d_valid, const void* d_coeffs, uint32_t sections, const void* d_gain,
                          int clamp, void* hip_stream);

/*
 * alacgpu_level_device: every crop brought to a known level, behind the noise mix and in front of the biquad cascade (no
 * counterpart in the reference): peak, RMS or ITU-R BS.1770-4 integrated loudness; two launches, no atomics, nothing read back,
 * the same inputs give the same bits.  The layout is planar float32: d_src and d_out [rows, channels, stride], the first
 * `frames` elements of a plane are data, what lies behind them is neither read nor written.  d_out is d_src itself (in
 * place), an array of that layout apart from it, or NULL: the row is then only measured.  The kernels evaluate no logarithm
 * and no power: `target` is linear and the caller's, as alacgpu_mix_device's ratio is.  For row r, with
 * v = min(max(d_valid[r], 0), frames) (int64 [rows]; NULL: frames), everything in float64 on x widened exactly:
 *   P = max |x[c, i]| over all channels and i < v                  (mode 0, 1, 2: peak, rms, lufs)
 *   peak: g = target / P                                           target: the peak to reach
 *   rms:  E = (sum over c, i < v of x^2) / (channels v),  g = sqrt(target / E)          target: the mean square, 10^(db / 10)
 *   lufs: every channel K-weighted by the two sections d_kweight (float64 [2, 5] = (b0, b1, b2, a1, a2): BS.1770's shelf and
 *     high-pass at the rate of the crops, designed by the caller), each from zero history, by alacgpu_biquad_device's blocked
 *     recurrence with nothing rounded to float32; s_c[k] the sum of its squares over hop k of `hop` frames (a tenth of a
 *     second), k < nh = v / hop; for block j < nh - 3 (four hops, starting every hop)
 *       z_c[j] = ((s_c[j] + s_c[j+1]) + (s_c[j+2] + s_c[j+3])) / (4 hop),   e[j] = sum over c of G_c z_c[j],   G = (1, 1, 1, 1.41, 1.41)
 *     E = the mean of the e[j] that are above Gabs = 10^((-70 + 0.691) / 10) and above 0.1 times the mean of those above Gabs,
 *     g = sqrt(target / E)                                         target: 10^((LUFS + 0.691) / 10)
 *   max_peak > 0: g = min(g, max_peak / P)
 *   y[c, i] = fl32(g * x[c, i]) for i < v, rounded once; with clamp then min(max(y, -1), 1), a NaN kept
 * Frames at or behind v are untouched (out of place too: d_out keeps what it held).  A row with nothing to measure -- v == 0,
 * P == 0, E == 0, for lufs fewer than 4 hops or no block above Gabs -- keeps g = 1 exactly and is neither read by the second
 * launch nor written, and so is a row whose g comes out exactly 1 without clamp.  d_gain_out, d_energy_out and d_peak_out
 * (float64 [rows], each may be NULL) receive g, E (the mean square in peak mode; 0 where there was nothing to gate) and P.
 * The first launch, one workgroup per (row, channel), walks the plane in tiles of 4096 frames, 16 consecutive frames a lane,
 * and writes the sum of squares, the peak and the hop sums into the ctx's scratch, float64 [rows, channels, 2 + frames / hop];
 * the second, a grid of rows times parts of 4096 frames (the smallest multiple that keeps a row within 256 parts), combines
 * its row's scratch in every workgroup and writes its part of y.  The order of every sum is fixed and does not depend on
 * the width of the loads (csrc/alac_level.h states it, alac.net_amd/level.py follows it operation by operation): a lane's 16
 * squares in ascending order; for the sum of squares the lanes of a wave and the waves as trees of halves and the tiles in
 * ascending order; for a hop the partials of its chunks in ascending order, a chunk that straddles a hop boundary giving its
 * first frames to one hop and its last to the next; blocks and channels in ascending order.  One correctly rounded division
 * and root, no multiply fused into an add.  Anything else follows IEEE: a NaN or an infinity in x below v reaches its own row
 * only (a NaN peak or energy makes g a NaN; a block whose energy is a NaN is above no gate); one at or behind v is never read.
 * Loads and stores are 16 bytes wide where the bases and the stride are multiples of 16 bytes, single frames otherwise, with
 * the same result.  Calls of one ctx share the scratch one after the other, whatever their streams (as alacgpu_mix_device's
 * do).  Device pointers only, asynchronous on hip_stream.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or d_src, a NULL d_kweight for lufs, a NULL d_out with all three
 * outputs NULL, a misaligned array (4; 8 for d_valid, d_kweight and the three outputs), a mode above 2, channels 0 or above 5
 * for lufs, hop below 16 for lufs, frames 0 or above stride, a target that is not positive and finite, a max_peak that is not
 * finite, d_src and d_out that overlap without being equal, an output overlapping d_src or d_out, d_kweight overlapping d_out,
 * an extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_level_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t stride,
                         uint64_t frames, const void* d_valid, uint32_t mode, uint32_t hop, const void* d_kweight, double target,
                         double max_peak, int clamp, void* d_gain_out, void* d_energy_out, void* d_peak_out, void* hip_stream);

/*
 * alacgpu_yin_device: the fundamental frequency of the crops, frame by frame (no counterpart in the reference): the YIN
 * estimator of de Cheveigne and Kawahara (JASA 2002), steps 1 to 5; one launch, no atomics, no scratch, the same inputs give
 * the same bits.  d_src is planar float32 [rows, channels, stride], the first `frames` elements of a plane are data, what lies
 * behind them is not read; d_out is float32 [rows, channels, 2, out_frames], apart from d_src.  For row r, with v =
 * min(max(d_valid[r], 0), frames) (int64 [rows]; NULL: frames), span = win_length + tau_max, samples outside [0, v) reading as
 * zero, the row has v / hop + 1 frames centred on c_t = t hop (align_length 0), or 1 + (v - align_length) / hop frames, none
 * for v < align_length, centred on c_t = t hop + align_length / 2; frame t starts at s = c_t - span / 2, and
 *   d[tau]  = sum_{j < win_length} (x[s + j] - x[s + j + tau])^2                      tau = 0 .. tau_max, the direct sum
 *   d'[tau] = d[tau] tau / (d[1] + .. + d[tau]), 1 where that sum is 0; d'[0] = 1
 *   tau     = the first of tau_min .. tau_max - 1 with d'[tau] < threshold, then forward while d'[tau + 1] < d'[tau] (up to
 *             tau_max - 1); without one the first argmin of d' over that range (a NaN as +infinity)
 *   shift   = (a - c) / (2 (a - 2 b + c)) for (a, b, c) = d'[tau - 1 .. tau + 1] when b <= a, b <= c and a - 2 b + c > 0, else 0
 *   out[r, ch, 0, t] = sample_rate / (tau + shift),  out[r, ch, 1, t] = b           f0 in Hz, and the aperiodicity
 * and (0, 1) for a frame whose d[1] + .. + d[tau_max] is 0 (silence, a constant).  The frame is voiced exactly when its
 * aperiodicity is below the threshold.  Frames at and behind the row's count, up to out_frames, are zero in both lines.  A
 * workgroup of 256 lanes takes a plane and a tile of up to 8 consecutive frames, whose samples it loads once into LDS; every
 * lag's sum runs over j in ascending order as e = fl(x[s + j] - x[s + j + tau]), acc = fma(e, e, acc); a wave per frame then
 * scans the lags in chunks of 64 and searches.  Every other operation is one IEEE float32 operation, the divisions correctly
 * rounded (csrc/alac_yin.h and alac.net_amd/yin.py state the order; the twin there equals the kernel bit for bit, and the
 * module derives how far any float32 evaluation may be from the exact one).  Anything else follows IEEE: a NaN sample makes d'
 * NaN from the first lag whose sum reaches it, in the frames whose span holds it, and no other.  Nothing of the ctx is used but
 * its device, so calls on different streams are independent.  Device pointers only, asynchronous on hip_stream, nothing is
 * read back.  rows == 0 or out_frames == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_out, a misaligned array (4; 8 for d_valid), channels
 * 0, frames 0 or above stride, sample_rate 0, hop 0, a win_length that is no multiple of 64 in 64 .. 2048, tau_min below 2,
 * tau_max above 2048 or not above tau_min + 1, a threshold outside (0, 1], out_frames that is not the frame count of a row of
 * `frames` samples, d_src and d_out that overlap, an extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_yin_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                       const void* d_valid, uint32_t sample_rate, uint32_t win_length, uint32_t hop, uint32_t tau_min,
                       uint32_t tau_max, uint32_t align_length, float threshold, void* d_out, uint64_t out_frames,
                       void* hip_stream);

/*
 * alacgpu_pyin_device: the smoothed fundamental frequency of the crops (no counterpart in the reference): probabilistic YIN of
 * Mauch and Dixon (ICASSP 2014), what librosa.pyin computes -- per frame the troughs of alacgpu_yin_device's d' with a
 * probability each, then a Viterbi decode over 2 n_bins states (voiced and unvoiced pitch bins) along every plane.  Two
 * launches, no atomics, the same inputs give the same bits.  d_src, d_valid, sample_rate, win_length, hop, tau_min, tau_max,
 * align_length and the frames of a row are alacgpu_yin_device's.  d_table is the float32 tables of the specification, packed
 * in the order of alac_pyin_tables (csrc/alac_pyin.h) for n_thresholds thresholds, (tau_max - tau_min + 1) / 2 troughs at most,
 * n_bins bins and a transition band of `band` = min(h, n_bins - 1) bins to either side; alac.net_amd/pyin.py states the tables,
 * every operation in order, the tie rule (the lowest source state) and the bounds, and its twin equals the kernels bit for bit.
 *   stage 0  both launches: d_out is float32 [rows, channels, 3, out_frames], apart from d_src: the decoded bin's frequency in
 *            Hz, 1 where the state is voiced and 0 where not, the voicing probability; zeros at and behind a row's frame
 *            count.  The log2 observations (float32 [planes, out_frames, n_bins + 2]) and the uint16 backpointers
 *            ([planes, out_frames, 2 n_bins]) lie in a scratch of the ctx that its calls share one after the other, whatever
 *            their streams.  The other four arrays are not used.
 *   stage 1  the observation alone, into d_obs_voiced float32 [rows, channels, out_frames, n_bins], d_obs_unvoiced and d_vp
 *            [rows, channels, out_frames]; zeros at and behind a row's frame count.  No scratch.
 *   stage 2  the decode alone, on d_obs_voiced and d_obs_unvoiced as stage 1 leaves them (finite values), into d_states int32
 *            [rows, channels, out_frames]: the path, -1 at and behind a row's count.  d_valid then holds FRAMES per row
 *            (NULL: out_frames); d_src, stride and frames are not used.  The backpointers lie in the scratch.
 * A line without frames runs no recursion.  Device pointers only, asynchronous on hip_stream, nothing is read back.  rows == 0
 * or out_frames == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, a stage outside 0 .. 2, a NULL among the arrays the stage uses
 * (d_table always), a misaligned array (4; 8 for d_valid), channels 0, sample_rate 0, hop 0, the win_length, tau_min and
 * tau_max alacgpu_yin_device refuses, n_thresholds outside 1 .. 256, n_bins outside 1 .. 1024, band not below n_bins,
 * no_trough_prob outside [0, 1], 2^31 planes or frames or more, a scratch above 2^31 bytes, and in stages 0 and 1 frames 0 or
 * above stride, out_frames that is not the frame count of a row of `frames` samples, d_src overlapping what is written, an
 * extent of 2^60 bytes or more, 2^31 workgroups or more.
 */
int alacgpu_pyin_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                        const void* d_valid, uint32_t sample_rate, uint32_t win_length, uint32_t hop, uint32_t tau_min,
                        uint32_t tau_max, uint32_t align_length, uint32_t n_thresholds, uint32_t n_bins, uint32_t band,
                        float no_trough_prob, const void* d_table, void* d_obs_voiced, void* d_obs_unvoiced, void* d_vp,
                        void* d_out, void* d_states, uint64_t out_frames, int stage, void* hip_stream);

/*
 * alacgpu_kaldi_pitch_device: Kaldi's pitch features of the crops (no counterpart in the reference): what
 * compute-kaldi-pitch-feats | process-kaldi-pitch-feats produce (Ghahremani et al., ICASSP 2014) -- the signal downsampled to
 * resample_freq, the NCCF of every frame interpolated onto a logarithmic lag grid of n_states states, a dense Viterbi decode
 * along every plane (a quadratic transition cost over ALL source states, every tie to the lowest), and the post-processing as
 * the decode's epilogue.  Three launches, no atomics, the same inputs give the same bits.  d_src is planar float32
 * [rows, channels, stride], the first `frames` elements of a plane are signal, of which a row's first
 * v = min(max(d_valid[row], 0), frames) count (d_valid NULL: frames).  win_length and hop are the frame and the shift in input
 * samples, window and shift those at resample_freq; a row of v samples has min(v < win_length ? 0 : 1 + (v - win_length) / hop,
 * n < window ? 0 : 1 + (n - window) / shift) frames, n = ceil(v resample_freq / sample_rate), and out_frames is that count of
 * `frames`.  d_table is the float32 tables of the specification, packed in the order of alac_kpitch_tables
 * (csrc/alac_kaldi_pitch.h) for `phases` phases of down_taps taps (an output sample n reads the input from
 * (n / phases) in_per_unit + first[n % phases] on), the integer lags first_lag .. last_lag, n_states states of up_taps
 * interpolation taps and 2 delta_window + 1 delta coefficients; alac.net_amd/kaldi_pitch.py states the tables, every operation
 * in order, the deviations from Kaldi and the bounds, and its twin equals the kernels bit for bit.  flags: 1 post-process, and
 * with it 2 the POV feature, 4 the normalised log-pitch (over left_context and right_context frames), 8 the delta (over
 * delta_window frames), 16 the raw log-pitch: `lines` is 2 without bit 1, else the number of bits 2 .. 16 set.
 *   stage 0  everything: d_out is float32 [rows, channels, lines, out_frames], apart from d_src: without post-processing the POV
 *            NCCF at the decoded lag and the pitch in Hz, else the lines asked for in Kaldi's order; zeros at and behind a row's
 *            frame count.  The downsampled rows, the NCCF planes and the uint16 backpointers ([planes, out_frames, n_states]) lie
 *            in a scratch of the ctx that its calls share one after the other, whatever their streams.
 *   stage 1  the downsampler and the NCCF alone, into d_nccf float32 [rows, channels, 2, out_frames, n_states], apart from d_src:
 *            the pitch NCCF (with the ballast) and the POV NCCF (without); zeros at and behind a row's frame count.
 *   stage 2  the decode alone, on d_nccf (finite values), into d_raw float32 [rows, channels, 2, out_frames]: stage 0's output
 *            without post-processing.  d_valid then holds FRAMES per row (NULL: out_frames); d_src, stride and frames are not used.
 *   stage 3  the post-processing alone (flags bit 1 must be set), on d_raw into d_out [rows, channels, lines, out_frames]; d_valid
 *            as in stage 2.
 * A line without frames runs no recursion.  Device pointers only, asynchronous on hip_stream, nothing is read back.  rows == 0
 * or out_frames == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, a stage outside 0 .. 3, a NULL among the arrays the stage uses
 * (d_table always), a misaligned array (4; 8 for d_valid), channels 0, a rate, win_length, hop or shift of 0, resample_freq above
 * sample_rate, window below 2, first_lag 0, last_lag not above first_lag, n_states outside 1 .. 1024, phases, in_per_unit or
 * down_taps 0, more than 4096 downsampler weights, up_taps 0 or above the number of integer lags, a frame whose LDS image passes
 * 64 KiB, flags above 31 or post-processing without a line, stage 3 without post-processing, delta_window outside 1 .. 64, a
 * context above 2^20, 2^31 planes or frames or more, a scratch above 2^31 bytes, and in stages 0 and 1 frames 0 or above stride,
 * out_frames that is not the frame count of a row of `frames` samples, d_src overlapping what is written, an extent of 2^60
 * bytes or more, 2^31 workgroups or more; in stage 2 d_nccf overlapping d_raw, in stage 3 d_raw overlapping d_out.
 */
int alacgpu_kaldi_pitch_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                               const void* d_valid, uint32_t sample_rate, uint32_t resample_freq, uint32_t win_length, uint32_t hop,
                               uint32_t window, uint32_t shift, uint32_t first_lag, uint32_t last_lag, uint32_t n_states,
                               uint32_t phases, uint32_t in_per_unit, uint32_t down_taps, uint32_t up_taps, uint32_t flags,
                               uint32_t left_context, uint32_t right_context, uint32_t delta_window, const void* d_table,
                               void* d_nccf, void* d_raw, void* d_out, uint64_t out_frames, int stage, void* hip_stream);

/*
 * alacgpu_cqt_device: constant-Q features of the crops (no counterpart in the reference): the direct constant-Q transform,
 * every bin's own windowed complex exponential against the signal; one launch, no atomics, no scratch, the same inputs give the
 * same bits.  d_src is planar float32 [rows, channels, src_stride], the first `frames` elements of a plane are signal, zeros
 * are read outside them and nothing is reflected; d_out is float32 [rows, channels, n_bins, out_frames], out_frames =
 * 1 + frames / hop, every element written.  Frame t is centred on sample t hop; with N_k = lengths[k] (host memory, uint32
 * [n_bins], falling with k, 2 .. 36864; d_lengths is the same array in device memory) and c_k = N_k / 2,
 *   C[k, t] = sum over n < N_k of g_k[n] x[t hop - c_k + n],   P = Re(C)^2 + Im(C)^2,
 *   out[k, t] = sqrt(P) (power 1) or P (power 2); log_mode 1 or 2: ln or log10 of max(that, floor)
 * d_table holds the g_k as float32 in blocks of 16 bins: block b is [K_b][32], K_b the even number at or above N_{16 b}, row r
 * the real ((r >> 3) & 1 == 0) or imaginary part of the block's bin (r >> 4) 8 + (r & 7), bin k's taps at n' = c_{16 b} - c_k + n
 * with zeros around them (alac.net_amd/cqt.py builds it and states the arithmetic, csrc/alac_cqt.h the layout).  A workgroup
 * of 256 lanes takes a plane and a tile of up to 32 frames, whose span it loads once into LDS; a block is one accumulator of
 * v_mfma_f32_32x32x2_f32 over its K_b taps: k-ordered chains of float32 fused multiply-adds, P = fma(re, re, round(im im)),
 * the root correctly rounded.  A NaN or an infinity reaches element (k, t) exactly through bin k's own taps of frame t (a
 * tile whose span holds one is evaluated bin by bin); every other element is what it is without it.  Nothing of the ctx is
 * used but its device, so calls on different streams are independent.  Device pointers (but `lengths`), asynchronous on
 * hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a misaligned array (4), channels 0, n_bins outside
 * 1 .. 512, hop outside 1 .. 2^20, lengths that rise, exceed 36864 or fall below 2, a power that is not 1 or 2, an unknown
 * log_mode, a floor that is not positive and finite, frames 0 or above src_stride, out_frames that is not 1 + frames / hop,
 * 2^31 workgroups or more.
 */
int alacgpu_cqt_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                       uint32_t hop, uint32_t n_bins, const uint32_t* lengths, const void* d_lengths, const void* d_table, int power,
                       int log_mode, float floor, void* d_out, uint64_t out_frames, void* hip_stream);

/*
 * alacgpu_stft_device: linear, complex or banded (mel) spectrograms of the crops (no counterpart in the reference): the
 * short-time Fourier transform by an FFT; one launch, no atomics, no scratch, the same inputs give the same bits.  d_src is
 * planar float32 [rows, channels, src_stride], the first `frames` elements of a plane are signal; d_out is float32 [rows,
 * channels, lines, out_frames], out_frames = 1 + frames / hop, every element written.  n_fft is 256, 512, 1024 or 2048,
 * n_bins = n_fft / 2 + 1.  Frame t is centred on sample t hop and reflected once at both ends as alacgpu_logmel_device's:
 *   X_t[k] = sum over n < n_fft of d_window[n] x_t[n] exp(-2 pi i k n / n_fft),   k < n_bins
 * d_window is float32 [n_fft] (a shorter window stands at offset (n_fft - win_length) / 2 with zeros around it), d_table is
 * float32 [n_fft][2], (cos, -sin)(2 pi k / n_fft).  power 0: the complex spectrum, lines = 2 n_bins, the real parts in the
 * lines 0 .. n_bins, the imaginary parts behind them (fb_lines 0 and log_mode 0 then); power 1: |X|; power 2: |X|^2, lines =
 * n_bins.  fb_lines in 1 .. 256: a filterbank on that, lines = fb_lines: line m is the sum over i < count_m of
 * d_weights[offset_m + i] v[first_m + i], with `bands` (host memory, uint32 [fb_lines][3]: first, count, offset; d_bands is
 * the same array in device memory) naming each line's band of bins and where its weights begin in d_weights, packed in the
 * order of the lines; a count of 0 gives 0.  log_mode 1 or 2: ln or log10 of max(that, floor).  The frames 2 j and 2 j + 1
 * of a plane are the real and imaginary part of one complex n_fft-point transform in LDS; a workgroup takes a tile of 8 to 64
 * consecutive frames of a plane and stores whole runs of a line (alac.net_amd/stft.py states the arithmetic operation by
 * operation, csrc/alac_stft.h the tile).  A NaN or an infinity reaches the two frames of the pair that holds it and no other.
 * Nothing of the ctx is used but its device, so calls on different streams are independent.  Device pointers (but `bands`),
 * asynchronous on hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array (the three of the filterbank may be NULL with fb_lines
 * 0), a misaligned array (4; d_table 8), channels 0, another n_fft, hop outside 1 .. n_fft, frames below n_fft / 2 + 1 or above
 * src_stride, out_frames that is not 1 + frames / hop, fb_lines above 256, a band that leaves 0 .. n_bins or whose offset is
 * not the sum of the counts before it, a power that is not 0, 1 or 2, power 0 with a filterbank or a log, an unknown log_mode,
 * a floor that is not positive and finite, 2^31 workgroups or more.
 */
int alacgpu_stft_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                        uint32_t n_fft, uint32_t hop, const void* d_window, const void* d_table, int power, uint32_t fb_lines,
                        const uint32_t* bands, const void* d_bands, const void* d_weights, int log_mode, float floor, void* d_out,
                        uint64_t out_frames, void* hip_stream);

/*
 * alacgpu_reverb_device: room reverberation into the crops, in front of the noise mix (no counterpart in the reference): every
 * crop convolved with its own impulse response by a uniformly partitioned overlap-save convolution; two launches, no atomics,
 * the same inputs give the same bits.  The layout is planar float32: d_src and d_out [rows, channels, stride], d_rir [rows,
 * rir_channels, rir_stride] with rir_channels 1 (the one channel goes into every channel of the signal) or channels; the first
 * `frames` (`rir_frames`) elements of a plane are data, what lies behind them is neither read nor written.  d_out is d_src
 * itself (in place) or an array of that layout apart from it.  For row r, with v = min(max(d_valid[r], 0), frames) and
 * vh = min(max(d_rir_valid[r], 0), rir_frames) (int64 [rows]; NULL: frames, rir_frames),
 *   d = the first k < vh at which |h[0, k]| is largest          the direct path; channel 0 decides for every channel
 *   e = (sum over c < rir_channels, k < vh of h[c, k]^2) / rir_channels,  g = 1 / sqrt(e)       one gain for every channel
 *   y[c, i] = g * sum over k < vh of h[c mod rir_channels, k] * x[c, i + d - k]   for i < v, x taken as 0 outside 0 .. v
 *   y[c, i] = x[c, i]                                                              for v <= i < frames (in place: untouched)
 * The result is as long as the crop and aligned on the direct path; the tail behind v is dropped.  A row with v == 0, with
 * vh == 0 ("no reverberation for this crop"), with e == 0 (a silent response) or with an e that is not finite is left as it
 * is bit for bit (in place: nothing is written), and only the analysis reads its response.  A NaN or an infinity in x below v
 * reaches that row and no other (one in h below vh makes e not finite: the row stays); one at or behind v (vh) is never read.
 * The arithmetic is float32, every operation rounded once, none fused, division and root correctly rounded: blocks of 4096
 * frames at a hop of 2048, transformed as 4096 complex points by a radix-4 transform in LDS whose twiddles are a table made in
 * double precision and rounded once; the response is cut into ceil(vh / 2048) partitions.  The first launch writes the spectrum
 * of every block of every signal plane and of every partition of every response plane, and per row d, g and the verdict, into
 * the ctx's scratch (8 * 4096 bytes a spectrum: rows * (channels * (ceil(frames / 2048) + 1) + rir_channels *
 * ceil(rir_frames / 2048)) spectra); the sum of squares is float32 in a fixed order: partial t of 256 takes the frames t,
 * t + 256, ... of channel 0, then of channel 1, and the 256 partials are added as a tree of halves (q[t] += q[t + s],
 * s = 128 .. 1).  The second launch, one workgroup per row, channel and block of 2048 outputs, adds X[m - p] . H[p] over the
 * partitions in ascending p, transforms back once, and stores g * w[i + d] over i < v.  csrc/alac_reverb.h states the
 * transform and the layout.  Calls of one ctx share the scratch one after the other, whatever their streams (as
 * alacgpu_mix_device's do); the first call of a ctx uploads the twiddle table with a blocking copy.  Device pointers only,
 * asynchronous on hip_stream, nothing is read back.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out or d_rir, a misaligned array (4; 8 for d_valid and
 * d_rir_valid), channels 0, rir_channels neither 1 nor channels, frames 0 or above stride, rir_frames 0 or above rir_stride,
 * d_src and d_out that overlap without being equal, d_rir overlapping d_out, an extent of 2^60 bytes or more, 2^31 workgroups
 * or more in either launch.
 */
int alacgpu_reverb_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, const void* d_rir, uint32_t rows, uint32_t channels,
                          uint32_t rir_channels, uint64_t stride, uint64_t rir_stride, uint64_t frames, uint64_t rir_frames,
                          const void* d_valid, const void* d_rir_valid, void* hip_stream);

/*
 * alacgpu_rir_shoebox_device: room impulse responses of shoebox rooms by the image-source method, what alacgpu_reverb_device
 * convolves a crop with where there is no recorded response (no counterpart in the reference); one launch, no atomics, no
 * scratch, nothing read back, the same inputs give the same bits.  d_geometry float64 [rows, 9]: the room (Lx, Ly, Lz), the
 * source and the microphone in metres; d_beta float32 [rows, 6]: the reflection coefficients of the walls at 0 and at L_a of
 * the axes x, y, z; d_out float32 [rows, out_stride] of which the first `frames` of a row are written; d_lengths int32 [rows].
 * Image (n, p), n in Z^3, p in {0, 1}^3, has the coordinate (1 - 2 p_a) s_a + 2 n_a L_a - r_a on axis a, the distance d, the
 * delay tau = d sample_rate / sound_speed, the order sum |2 n_a - p_a| and the amplitude
 * A = prod beta[a][0]^|n_a - p_a| beta[a][1]^|n_a| / (4 pi d), and
 *   h[k] = sum over the images with |k - tau| < taps / 2 of A * 0.5 (1 + cos(2 pi t / taps)) * sinc(t),  t = k - tau,  k < frames
 * in ascending (nx, ny, nz, 4 px + 2 py + pz); max_order -1 takes every order, else only images of an order up to it.
 * d_lengths[r] = frames.  A row is refused -- zeros, d_lengths[r] = 0, which alacgpu_reverb_device leaves alone -- where one of
 * its nine numbers is not finite, a dimension is not positive, the source or the microphone lies outside the room, or the
 * candidate box 8 (2 Nx + 1)(2 Ny + 1)(2 Nz + 1), N_a = floor((frames + taps) / (sample_rate / sound_speed) / (2 L_a)) + 2 (with
 * max_order at most (max_order + 1) / 2), exceeds 2^25 or a quotient 2^20: decided in the kernel.  An image at d == 0 gives an
 * infinity.  The geometry of an image is float64, a tap's arithmetic float32 from explicit polynomials, every operation rounded
 * once, none fused; csrc/alac_rir.h states the scheme, alac.net_amd/rir.py every operation and the derived bound.  Device
 * pointers only, asynchronous on hip_stream.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx or array, a misaligned array (8 for d_geometry, 4), sample_rate 0
 * or above 2^31 - 1, frames 0, above 2^20 or above out_stride, taps even or outside 3 .. 127, max_order below -1, a sound_speed
 * that is not positive and finite, arrays that overlap d_out or d_lengths, 2^31 workgroups or more.
 */
int alacgpu_rir_shoebox_device(alacgpu_ctx* ctx, const void* d_geometry, const void* d_beta, uint32_t rows, uint32_t sample_rate,
                               uint64_t frames, uint32_t taps, int32_t max_order, double sound_speed, void* d_out, uint64_t out_stride,
                               void* d_lengths, void* hip_stream);

/*
 * alacgpu_time_stretch_device: time stretch of the crops with the pitch kept, a phase vocoder (no counterpart in the reference;
 * the specification is torchaudio's phase_vocoder with the STFT and iSTFT around it); three launches, no atomics, nothing read
 * back, the same inputs give the same bits.  Followed by alacgpu_resample_ratio_rows_device at the same ratio it is a pitch
 * shift.  The layout is planar float32: d_src [rows, channels, src_stride] of which the first `frames` of a plane are data,
 * d_out [rows, channels, out_stride] of which the first out_frames are written; the two are apart.  n_fft = N is 512, 1024 or
 * 2048, the hop H = N / 4, the window w[n] = 0.5 - 0.5 cos(2 pi n / N).  Row r with v = min(max(d_valid[r], 0), frames) (int64
 * [rows]; NULL: frames) is stretched by p / q = d_p[r] / d_q[r] (int32 [rows], output length over input length):
 *   T = 1 + v / H frames X_t = DFT(w[n] x[refl(t H - N / 2 + n)]), refl(i) = -i below 0, 2 (v - 1) - i from v on; two zero frames
 *     behind them;
 *   output frame j < T' = ceil(T p / q) reads i = (j q) / p and i + 1 with alpha = ((j q) % p) / p:
 *     Y_j = (alpha |X_{i+1}| + (1 - alpha) |X_i|) P_j,   P_0 = ph(X_0),   P_{j+1} = ph(P_j (ph(X_{i+1}) conj(ph(X_i)))),
 *     ph(z) = z / |z| and 1 where |z| is not above 0 -- the phase advance of torchaudio's vocoder modulo 2 pi, without an angle;
 *   sample n of the output is sum over the frames j < T' that cover it of w[i] IDFT(Y_j)[i], i = n + N / 2 - j H, divided by the
 *     sum of w[i]^2 over the same frames (at least 1.25), for n <= (T' - 1) H and n < Ls = (2 v p + q) / (2 q); zero from there
 *     up to out_frames.  (torch.istft divides the last N / 2 samples by envelopes down to 1e-11 instead.)
 * d_valid_out[r] (int64 [rows]) receives min(Ls, out_frames).  A row is left alone -- neither read nor written, and
 * d_valid_out[r] = min(d_valid[r], frames) -- where p == q, where v <= N / 2 (no reflection) and where p or q is outside
 * 1 .. 2^20.  The arithmetic is float32, every operation rounded once, none fused, division and root correctly rounded, in a
 * fixed order that csrc/alac_stretch.h states and alac.net_amd/pitch.py follows operation by operation: an N-point complex
 * transform in LDS (radix 4, for 512 and 2048 behind one radix-2 stage) whose twiddles and window are tables made in double
 * precision and rounded once; one lane per bin walks the output frames in ascending order; a workgroup per four hops of output
 * transforms the seven frames that cover them back and adds them in ascending order.  The spectra of the input and output
 * frames live in the ctx's scratch (8 bytes a bin, N / 2 + 1 bins a frame); calls of one ctx share it one after the other,
 * whatever their streams (as alacgpu_reverb_device's do); the first call of a ctx with an n_fft uploads its tables on
 * hip_stream.  A NaN or an infinity in x below v reaches its own plane only; one at or behind v is never read.  Device pointers
 * only, asynchronous on hip_stream.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out, d_p, d_q or d_valid_out, a misaligned array (4; 8
 * for d_valid and d_valid_out), another n_fft, channels 0, frames 0 or above src_stride, out_frames 0 or above out_stride,
 * either of 2^40 or more, arrays that overlap (but for d_src with d_p, d_q and d_valid), an extent of 2^60 bytes or more, 2^31
 * workgroups or more in a launch.
 */
int alacgpu_time_stretch_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels,
                                uint64_t src_stride, uint64_t out_stride, uint64_t frames, uint64_t out_frames, const void* d_p,
                                const void* d_q, const void* d_valid, void* d_valid_out, uint32_t n_fft, void* hip_stream);

/*
 * alacgpu_copy_rows_device: the first v = min(max(d_valid[r], 0), frames) frames of every plane of row r copied from d_src
 * [rows, channels, src_stride] to d_out [rows, channels, out_stride] (planar float32, apart), nothing else written: how a
 * stage that works out of place -- the pitch shift: stretch, resample -- puts its rows back behind the lengths' guard.  d_valid:
 * int64 [rows].  One launch, no scratch, asynchronous on hip_stream.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src, d_out or d_valid, a misaligned array (4; 8 for d_valid),
 * channels 0, frames 0 or above either stride, d_src or d_valid overlapping d_out, an extent of 2^60 bytes or more, 2^31
 * workgroups or more.
 */
int alacgpu_copy_rows_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels,
                             uint64_t src_stride, uint64_t out_stride, uint64_t frames, const void* d_valid, void* hip_stream);

/*
 * alacgpu_specaugment_device: SpecAugment on the features, behind the normalisations (no counterpart in the reference): a time
 * warp, frequency masks and time masks per crop in one launch, no atomics, no scratch.  The data is float32 [rows, channels,
 * n_mels, line_stride]: a line is one mel bin of one channel of a row, its first line_len <= line_stride elements are
 * frames, what lies behind them is neither read nor written.  d_out is d_src itself (in place) or an array of the same layout
 * apart from it.  All lines of row r share its draws, int32 on the device: d_warp [rows, 2] = (c, c') (NULL: no warp in this
 * call), d_freq [rows, n_freq, 2] and d_time [rows, n_time, 2] = (first, width).  With tau = min(max(d_valid[r], 0),
 * line_len) (d_valid: int64 [rows]; NULL: line_len), in this order:
 *   warp    only where 1 <= c, c' <= tau - 2 and c != c'.  Frame t < tau reads the source position
 *             s(t) = t c / c'                                       for t <= c'
 *             s(t) = c + (t - c') (tau - 1 - c) / (tau - 1 - c')    for t >  c'
 *           as i = floor(s) and the remainder r over the denominator den, in integers:
 *             y[t] = x[i]                                  where r == 0 (x[i + 1] is not read; t = 0, c' and tau - 1 are such)
 *             y[t] = x[i] + f * (x[i + 1] - x[i]),  f = fl(r) / fl(den)      the division, the difference, the product and the
 *                                                                            sum each rounded once, nothing contracted
 *   freq    mask k sets every frame t < tau of the bins first .. first + width - 1 (within 0 .. n_mels - 1) to fill
 *   time    mask k sets the frames first .. first + width - 1 (within 0 .. tau - 1) of every bin to fill
 * A width <= 0 is no mask; (0, 0) is no warp.  Frames at and behind tau, and every row with d_valid[r] <= 0, stay bit for bit
 * (out of place: are copied).  A line of a row without a warp is neither read nor rewritten as a whole in place: its masked
 * spans are stored and nothing else is touched; a frequency-masked line is stored without being loaded.  A warped line is
 * held in LDS, its tau frames, before any of it is written, and the masks are applied while it is stored.  Lines of up to 256
 * frames are taken by a wave each, four to a workgroup, longer ones by a workgroup of 256 threads each; accesses are 16 bytes
 * wide where a line's address allows, and single frames in front of and behind those.  A line of more than 16384 frames cannot
 * be warped (64 KiB of LDS); masks alone have no such limit.  Device pointers only, asynchronous on hip_stream, nothing is read
 * back; nothing of the ctx is used but its device.  rows == 0: nothing happens.
 * ALACGPU_ERR_BAD_ARG, before anything is enqueued: a NULL ctx, d_src or d_out, d_freq NULL with n_freq != 0, d_time NULL with
 * n_time != 0, a misaligned array (4; 8 for d_valid), channels 0, n_mels 0, channels * n_mels of 2^32 or more, line_len 0 or
 * above line_stride, d_src and d_out that overlap without being equal, an extent of 2^60 bytes or more, 2^31 workgroups or
 * more, a fill that is not finite, more than 1024 masks of a kind, d_warp with line_len above 16384.
 */
int alacgpu_specaugment_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint32_t n_mels,
                               uint64_t line_stride, uint64_t line_len, const void* d_valid, const void* d_warp,
                               const void* d_freq, uint32_t n_freq, const void* d_time, uint32_t n_time, float fill,
                               void* hip_stream);

/* Single-packet drop-in for `int DecodeFrame(byte[] inbuffer, int[] outbuffer)` (AlacFile.cs:428):
 * writes the reference's own int[] layout (24-bit: one int per byte) and returns its byte count in
 * *out_bytes.  status as above (the C# shim rethrows the reference's exceptions from it). */
int alacgpu_decode_frame(alacgpu_ctx* ctx, uint32_t cfg_index, const uint8_t* inbuffer, uint32_t in_bytes,
                         int32_t* outbuffer, uint32_t out_capacity_ints, int32_t* out_bytes, int32_t* status);

/* Host-side reshape: canonical int32-per-sample -> the exact int[] DecodeFrame writes
 * (AlacFile.cs:390-395,:555-557 for 24-bit; identity for 16-bit).  Returns ints written. */
size_t alacgpu_expand_reference_layout(const alacgpu_cfg* cfg, const int32_t* pcm, int32_t n_samples,
                                       int32_t* ref_ints);

/* AlacContext.FormatSamples (AlacContext.cs:214-256): reference int[] -> little-endian PCM bytes. */
size_t alacgpu_format_samples(int bytes_per_sample, const int32_t* ref_ints, int32_t count_bytes, uint8_t* dst);

/* Kernel time of the most recent launch of this ctx, from HIP events recorded on the launch stream around it
 * (milliseconds; < 0 if unavailable).  Waits for that launch.  After a host-buffer call that was cut into ranges
 * this is the last range's launch. */
float alacgpu_last_kernel_ms(alacgpu_ctx* ctx);

/* Output layout of the batch entry points.  ALACGPU_OUT_INT32 (default): one int32 per sample, as documented
 * above.  ALACGPU_OUT_PACKED_LE: the bytes AlacContext.Read hands out -- AlacContext.FormatSamples
 * (AlacContext.cs:214-256) fused into the kernel's store: packet p's little-endian PCM (2 or 3 bytes per sample,
 * interleaved) starts at (uint8_t*)(pcm_out + p*slot_ints) and is out_bytes[p] long.  The slot stride is unchanged;
 * alacgpu_decode_batch then copies back only the part of each slot the widest stream cfg can fill (2 or 3 bytes per
 * slot int), the rest of the caller's slot is left untouched. */
enum { ALACGPU_OUT_INT32 = 0, ALACGPU_OUT_PACKED_LE = 1 };
int alacgpu_set_output_format(alacgpu_ctx* ctx, int format);

/* Pairing: alacgpu_decode_batch_device on up to 4096 packets remembers, per packet (its device address, its size, a hash of its
 * first 16 bytes), where channel B of a two-channel packet starts; a later call on the same resident packets decodes both channels
 * side by side in one pass instead of one after the other, and checks the remembered start against where channel A ended: a
 * packet whose bytes changed in place is decoded again the usual way, the output never depends on the memory being right.  On by
 * default; a context whose calls gain nothing from it (packets it never finds again, nothing it can pair, starts that keep being
 * wrong) stops the paired launch by itself after 16 calls and tries again 4096 calls later.  A call on packets it has not seen pays one
 * nearly empty launch.  Calls with a destination or a window, bigger batches and the host-buffer entry points do not pair.
 * alacgpu_pairing_stats: out[0] packets decoded paired, out[1] two-channel packets without a remembered start, out[2] packets
 * whose remembered start was wrong, since the context was made; waits for the device.  alacgpu_pairing_shift_starts moves every
 * remembered start one bit on (so that each is wrong): for tests of the check, waits for the device. */
int alacgpu_set_pairing(alacgpu_ctx* ctx, int on);
int alacgpu_pairing_stats(alacgpu_ctx* ctx, uint64_t* out);
int alacgpu_pairing_shift_starts(alacgpu_ctx* ctx);

/* Page-locked host memory for batch buffers (blob, offsets, pcm_out ...).  Optional -- every entry point takes ordinary memory
 * too -- but the faster choice: when pcm_out of alacgpu_decode_batch / alacgpu_decode_frame is page-locked (from here, from
 * hipHostMalloc, or registered with hipHostRegister) the kernels store the PCM straight into it while the batch decodes and
 * there is no download behind the decode (cfg2, 4096 packets: 3.55 / 2.39 ms int32 / packed against 3.70 / 2.50 ms from
 * ordinary memory); what a slot holds beyond the packet's own output is then left untouched.
 * ALACGPU_ZERO_COPY=0 in the environment keeps the copying path (A/B).  NULL on failure. */
void* alacgpu_alloc_pinned(size_t bytes);
void alacgpu_free_pinned(void* p);

const char* alacgpu_strerror(int rc);
const char* alacgpu_status_string(int status);
const char* alacgpu_last_error(alacgpu_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
