/*
 * vorbis_synth_hip.h — C-ABI of the MI355X-native batched Vorbis spectral-synthesis path.
 *
 * This is the drop-in boundary for ONE hot path of albertz/ParseOggVorbis: everything the reference
 * does per audio packet AFTER the entropy decode, i.e.
 *
 *   floor-1 amplitude unwrap + curve render   src/ParseOggVorbis.hpp:521-590, src/Utils.hpp:58-183
 *   nonzero-vector propagate                  src/ParseOggVorbis.hpp:1174-1180
 *   inverse channel coupling                  src/ParseOggVorbis.hpp:1213-1241
 *   floor x residue ("dot product")           src/ParseOggVorbis.hpp:1243-1255
 *   inverse MDCT                              src/mdct.cpp:433-527 (tables: src/mdct.cpp:88-127)
 *   window + overlap-add + PCM hand-off       src/ParseOggVorbis.hpp:837-886, 1008-1109
 *
 * The reference runs that per packet inside VorbisStream::parse_audio (hpp:1128-1274); a host decoder
 * that keeps the sequential Ogg/Huffman parse on the CPU calls vsyn_submit_* once per BATCH instead
 * (between hpp:1211 "after_residue" and hpp:1213), then replays hooks / ParseCallbacks::gotPcmData in
 * packet order.  Plain C: POD structs, raw pointers and sizes, int status + const char** error, no
 * C++/torch types, no exceptions across the boundary.  All compute is HIP on gfx950; there is no CPU
 * fallback — every entry point fails with VSYN_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef VORBIS_SYNTH_HIP_H_
#define VORBIS_SYNTH_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSYN_ABI_VERSION 5 /* 2: + residue VQ stage (vsyn_attach_vq, vsyn_vq_batch), page-locked host buffers; 3: + vsyn_pcm_abs_sum_host,
                              vsyn_pcm_fetch_host, VSYN_SUBMIT_KEEP_PCM (additive; the feature taps no longer force the staged kernels);
                              4: + vsyn_fused_paths (additive); 5: + VSYN_SUBMIT_PRE_KERNELS (additive); still 5: + the PCM
                              conditioning entry points (vsyn_pcm_cond, vsyn_pcm_condition_*, vsyn_pcm_cond_spectral_host; additive) */

#define VSYN_MAX_CHANNELS 32 /* floor_used is a 32-bit mask (reference: uint8_t audio_channels) */
#define VSYN_MAX_POSTS 65    /* Vorbis I: 2 + 31 partitions x <=8 dims, capped at 65 by the spec */
#define VSYN_MIN_BLOCKSIZE 64
#define VSYN_MAX_BLOCKSIZE 8192 /* hpp:1294-1296 */

/* status codes (return value of every int function; 0 = ok, like ogg_vorbis_full_read, ParseOggVorbis.cpp:12-42) */
enum {
  VSYN_OK = 0,
  VSYN_ERR_INVALID = 1,   /* bad argument / bad setup (the reference's CHECK(...) on setup fields) */
  VSYN_ERR_NO_DEVICE = 2, /* no HIP device, or not gfx950-compatible code object */
  VSYN_ERR_HIP = 3,       /* a HIP runtime call failed; text in *err */
  VSYN_ERR_STREAM = 4     /* the batch itself is bad (see vsyn_status.flags) */
};

/* vsyn_status.flags — conditions on which the reference fails a CHECK and aborts the read (VSYN_ST_WINDOW_FLAGS: see there) */
enum {
  VSYN_ST_FLOOR_RANGE = 1u << 0,   /* predicted > range, hpp:536 */
  VSYN_ST_FLOOR_VALUE = 1u << 1,   /* rendered floor value >= 256, hpp:587 */
  VSYN_ST_GRANULE = 1u << 2,       /* page granule behind/ahead of what the packets provide, hpp:1029,1041 */
  VSYN_ST_PLANE_OVERFLOW = 1u << 3,/* a segment emits more than plane_stride samples (nothing is written out of bounds) */
  VSYN_ST_BAD_MODE = 1u << 4,      /* mode index >= num_modes */
  VSYN_ST_BAD_SEGMENT = 1u << 5,   /* segment out of range / unknown stream slot / unaligned residue_off */
  VSYN_ST_BAD_VQ = 1u << 6,        /* VQ stage: entry or classification number out of range, or entry count inconsistent with the classifications */
  VSYN_ST_WINDOW_FLAGS = 1u << 7   /* a block smaller than the long block in front of it, whose next_long flag is set (only possible when
                                      blocksize0 < blocksize1). Unlike the bits above, the reference ACCEPTS this input: it picks windows
                                      from the flags alone (hpp:874-886) and keeps the long window's right slope beyond the smaller block
                                      in its sliding buffer, where later packets add to it depending on when the buffer slides (hpp:1069-1109).
                                      The device refuses the packet rather than return different PCM. Every other flag combination is exact. */
};

/* ---- stream setup: the part of VorbisStreamSetup (hpp:889-964) the synthesis half reads ---- */

typedef struct vsyn_floor1 {          /* VorbisFloor1, hpp:416-471 */
  uint32_t multiplier;                /* 1..4 (hpp:446) */
  uint32_t num_posts;                 /* xs.size(), 2..65 */
  const uint32_t* xs;                 /* header order: xs[0]=0, xs[1]=1<<rangebits, then partition posts (hpp:448-456) */
} vsyn_floor1;

typedef struct vsyn_coupling {        /* VorbisMapping::Coupling, hpp:767 */
  uint16_t magnitude, angle;
} vsyn_coupling;

typedef struct vsyn_mapping {         /* VorbisMapping, hpp:765-814 */
  uint32_t num_couplings;
  const vsyn_coupling* couplings;     /* in header order; applied in reverse (hpp:1214) */
  const uint8_t* channel_floor;       /* [channels]: submaps[muxs[ch]].floor (hpp:1162-1163) */
} vsyn_mapping;

typedef struct vsyn_mode {            /* VorbisModeNumber, hpp:816-835 */
  uint8_t block_flag;                 /* 1 = long window (blocksize1) */
  uint8_t mapping;
} vsyn_mode;

typedef struct vsyn_setup {
  uint32_t channels;                  /* VorbisIdHeader.audio_channels, 1..VSYN_MAX_CHANNELS */
  uint32_t blocksize0, blocksize1;    /* powers of two, 64..8192, blocksize0 <= blocksize1 (hpp:1294-1298) */
  uint32_t num_floors;   const vsyn_floor1* floors;   /* all type 1 (type 0 is unimplemented upstream, hpp:402) */
  uint32_t num_mappings; const vsyn_mapping* mappings;
  uint32_t num_modes;    const vsyn_mode* modes;
} vsyn_setup;

/* ---- a batch ---- */

typedef struct vsyn_packet {          /* what hpp:1142-1172 leaves behind for one audio packet; 16 bytes */
  uint8_t mode;                       /* mode_idx, hpp:1146 */
  uint8_t prev_long, next_long;       /* prev/next window flags, hpp:1151-1152 (ignored for short blocks) */
  uint8_t reserved0;
  uint32_t floor_used;                /* bit c = VorbisFloor1::decode set use_output for channel c (hpp:478-482) */
  int64_t granule;                    /* setExpectedEndingPos(): page granule if last packet on its page, else -1 (hpp:1456-1459) */
} vsyn_packet;

#define VSYN_SEG_RESET 1u             /* segment starts a stream: no overlap carry-in, first packet emits nothing (hpp:1021) */

typedef struct vsyn_segment {         /* consecutive packets of one stream inside a batch; 24 bytes */
  uint32_t stream;                    /* stream slot, < max_streams; carries overlap state between submits */
  uint32_t first_packet;              /* index into packets[] / ys rows */
  uint32_t num_packets;
  uint32_t flags;                     /* VSYN_SEG_* */
  uint64_t residue_off;               /* float index of this segment's first residue block (multiple of 4) */
} vsyn_segment;

/*
 * Batch tensors (host or device resident depending on the entry point):
 *   packets  [P]                      vsyn_packet
 *   segments [S]                      vsyn_segment; segments must not overlap, a stream slot at most once per batch
 *   ys       [P][channels][ys_stride] uint16  coded floor-1 Y values ("floor1 ys", hpp:518); row ignored if !floor_used
 *   residue  packed float32: packet p of a segment, channel c, bin i at
 *              seg.residue_off + (sum of channels*n_q/2 over earlier packets q of the segment) + c*n_p/2 + i
 *            = "after_residue" (hpp:1211), length n_p/2 per channel
 *   pcm      [S][channels][plane_stride] float32, planar; segment g writes its emitted samples from offset 0
 *   emit_len [P] uint32 (optional)    samples per channel emitted for packet p = num_frames of forwardReadyPcm (hpp:1019-1059)
 */
typedef struct vsyn_taps {            /* optional debug taps = the reference's push_data_* hooks on this path */
  float* after_envelope;              /* same packing as residue; "after_envelope", hpp:1254 */
  float* pcm_after_mdct;              /* packed like residue with n_p per channel (2x offsets); "pcm_after_mdct", hpp:1265 */
  uint16_t* floor_final;              /* [P][channels][ys_stride]: final_y*multiplier | step2_flag<<15 ("floor1 final_ys"/"step2_flag", hpp:560-561) */
  uint16_t* floor_curve;              /* packed like residue (n_p/2 per channel): the rendered integer floor curve, "floor1 floor"
                                         (hpp:585; the reference's vector has n_p entries: the second half is flat at the last flagged post's y, hpp:583-584);
                                         with after_residue these are the feature tensors of returnn_import.py:74-115.
                                         Rows of channels without a decoded floor are left untouched */
} vsyn_taps;
/* after_envelope / pcm_after_mdct exist only in the staged (any-shape) kernels: asking for either routes the batch through them.
 * The two feature taps do not: floor_final comes from the unwrap kernel, floor_curve from the tap variant of the fused kernel. */

typedef struct vsyn_status {
  uint32_t flags;                     /* VSYN_ST_* OR-ed over the batch */
  uint32_t first_bad_packet;          /* lowest packet index that raised a flag (0xFFFFFFFF if none) */
} vsyn_status;

typedef struct vsyn_handle vsyn_handle;

/* submit flags */
#define VSYN_SUBMIT_STAGED 1u         /* force the staged (tap-capable, any-shape) kernels instead of the fused one */
#define VSYN_SUBMIT_INPUTS_READY 2u   /* vsyn_submit_device: packets/segments/ys are complete already (not produced by work still
                                         pending on hip_stream). Where a submit's preparation consists of the chained layout + floor-unwrap
                                         kernels (staged work, the VQ stage, very long segments, VSYN_SUBMIT_PRE_KERNELS), this lets them
                                         overlap the synthesis kernel of the previous submit; results are identical either way. */

#define VSYN_SUBMIT_PRE_KERNELS 8u    /* diagnostics / A-B: prepare the batch (layout scan, floor-1 step 1) with the two chained kernels also
                                         where the single dependency-free preparation kernel is the default (submits whose runs are all
                                         taken by the fused kernels); with VSYN_SUBMIT_INPUTS_READY they run hidden beside the previous
                                         submit's synthesis kernel (the default of rounds 1-3 for such submits); results are identical. */
#define VSYN_SUBMIT_KEEP_PCM 4u        /* vsyn_submit_host*: leave the PCM on the device (`pcm` may be NULL, nothing is copied back);
                                         fetch it in the form the consumer wants with vsyn_pcm_fetch_host */

const char* vsyn_version(void);
int vsyn_abi_version(void);

/* Builds the per-stream constant block (IMDCT twiddles for both blocksizes, the 1+4 window tables of
 * VorbisModeNumber::precalc hpp:837-862, floor-1 sorted posts + neighbour tables, coupling/mode tables,
 * inverse-dB table) on `device` and allocates overlap state for max_streams stream slots. */
int vsyn_create(const vsyn_setup* setup, int device, uint32_t max_streams, vsyn_handle** out, const char** err);
void vsyn_destroy(vsyn_handle* h);

uint32_t vsyn_ys_stride(const vsyn_handle* h);           /* uint16 elements per (packet,channel) row of ys */
uint32_t vsyn_channels(const vsyn_handle* h);
/* Which synthesis kernels this handle's setup gets (diagnostics, tests): bit 0 = the fused kernel takes runs of long blocks,
 * bit 1 = it also takes mixed-block runs and carry-ins; neither = every batch goes through the staged (any-shape) kernels.
 * Bit 8 (after vsyn_attach_vq) = the residue VQ kernel keeps the attached setup's value tables in LDS (they fit) instead of
 * gathering them from global memory. Results are the same either way; only the speed differs.
 * Neither of bits 0 / 1 also for a floor whose X list leaves the domain in which the fused kernels' float32 floor curve is proven
 * exact (x[1] = 1 << rangebits far beyond the half block, e.g. 32768): the staged kernels render the curve in integers. */
uint32_t vsyn_fused_paths(const vsyn_handle* h);
/* size in bytes of the constant block, and a copy of it (for the one RCCL broadcast of a multi-GPU job) */
size_t vsyn_const_block_bytes(const vsyn_handle* h);

/* All pointers are DEVICE pointers on the handle's device; asynchronous on hip_stream (a hipStream_t, NULL = default stream).
 * max_seg_packets >= every segment's num_packets (0 = num_packets); a longer segment gets no rows and raises VSYN_ST_BAD_SEGMENT.
 * Errors found on the device are reported by vsyn_sync_status. The features entry points of one handle share its feature
 * workspace and its status word (with the synthesis submits): issue them on one stream, or serialise them; vsyn_sync_status and
 * vsyn_features_host return every flag raised on the handle since the last read. */
int vsyn_submit_device(vsyn_handle* h,
                       uint32_t num_packets, const vsyn_packet* d_packets,
                       uint32_t num_segments, const vsyn_segment* d_segments, uint32_t max_seg_packets,
                       const uint16_t* d_ys, const float* d_residue,
                       float* d_pcm, uint64_t plane_stride,
                       uint32_t* d_emit_len, const vsyn_taps* d_taps,
                       uint32_t flags, void* hip_stream, const char** err);

/* Same with HOST pointers: stages to the device, runs, copies pcm / emit_len / taps back, synchronises (on a stream owned
 * by the handle: calls on different handles from different host threads overlap),
 * and returns VSYN_ERR_STREAM (status filled) if the device flagged the batch. residue_floats = total floats in residue. */
int vsyn_submit_host(vsyn_handle* h,
                     uint32_t num_packets, const vsyn_packet* packets,
                     uint32_t num_segments, const vsyn_segment* segments,
                     const uint16_t* ys, const float* residue, size_t residue_floats,
                     float* pcm, uint64_t plane_stride,
                     uint32_t* emit_len, const vsyn_taps* taps,
                     uint32_t flags, vsyn_status* status, const char** err);

/* ---- residue VQ stage: the data-parallel half of the residue decode on the device ----
 *
 * The reference's residue decode (VorbisResidue::decode, hpp:670-762) interleaves a bit-serial part — Huffman decode of
 * one classification word per partition group and one codebook ENTRY NUMBER per vector (VorbisCodebook::decodeScalar,
 * hpp:286-301) — with a data-parallel part: look the entry's value vector up (lookup_table_, hpp:212-245, 367-374) and
 * add it into the residue vector (hpp:737-753), once per cascade pass, then de-interleave format 2 (hpp:687-693).
 * With this stage the host decoder keeps only the bit-serial part and ships per packet the classifications (u8) and
 * entry numbers (u16) instead of the expanded float vectors; the device rebuilds "after_residue" (hpp:1211) in the same
 * order of additions, i.e. bit-identical, and the synthesis kernels continue from there.
 */
typedef struct vsyn_codebook {        /* VQ side of VorbisCodebook, hpp:104-245 */
  uint32_t dimensions;                /* dimensions_ */
  uint32_t num_entries;               /* num_entries_ (<= 65536 for this stage) */
  const float* lookup;                /* lookup_table_: [num_entries][dimensions] value vectors, or NULL (lookup type 0: scalar-only book) */
} vsyn_codebook;

typedef struct vsyn_residue {         /* VorbisResidue, hpp:623-668 */
  uint32_t type;                      /* 0, 1 or 2 */
  uint32_t begin, end, partition_size;
  uint32_t num_classifications;       /* 1..64 */
  uint32_t classwords;                /* dimensions_ of the class codebook (classifications per codeword, hpp:703) */
  const int16_t* books;               /* [num_classifications][8]: codebook per cascade pass, -1 = none (hpp:651-659) */
} vsyn_residue;

typedef struct vsyn_vq_mapping {      /* the residue side of VorbisMapping, hpp:765-814 */
  uint32_t num_submaps;               /* 1..16 */
  const uint8_t* mux;                 /* [channels]: submap of each channel (muxs) */
  const uint8_t* submap_residue;      /* [num_submaps]: residue number of each submap */
} vsyn_vq_mapping;

typedef struct vsyn_vq_setup {
  uint32_t num_codebooks; const vsyn_codebook* codebooks;
  uint32_t num_residues;  const vsyn_residue* residues;
  uint32_t num_mappings;  const vsyn_vq_mapping* mappings;   /* same count and order as vsyn_setup.mappings */
} vsyn_vq_setup;

/* Per packet, in decode order (hpp:708-760). For each submap s = 0.. of the packet's mapping, with the channels whose
 * mux == s in channel order as j = 0..nch-1 (format 2: one virtual channel, always decoded, hpp:685-694):
 *   cls      nch x parts bytes, [j][partition]: the classification numbers (hpp:716-719); parts = (min(end,len) -
 *            min(begin,len)) / partition_size, len = n/2 (format 2: nch*n/2). Rows of unused channels are present, ignored.
 *   entries  for pass 0..7, partition 0..parts-1, j 0..nch-1 (used channels with a codebook in that pass only):
 *            partition_size / dimensions entry numbers (hpp:741, 749) */
typedef struct vsyn_vq_packet {       /* 16 bytes */
  uint64_t entry_off;                 /* index of the packet's first entry in entries[] */
  uint32_t num_entries;
  uint32_t cls_off;                   /* index of the packet's first byte in cls[] */
} vsyn_vq_packet;

typedef struct vsyn_vq_batch {        /* host or device pointers, like the other batch tensors of the call */
  const vsyn_vq_packet* packets;      /* [P] */
  const uint8_t* cls;
  const uint16_t* entries;
  uint64_t num_cls, num_entries;      /* array lengths (bounds for validation / staging) */
} vsyn_vq_batch;

/* Uploads the codebook value tables and residue descriptions. VSYN_ERR_INVALID (with the reason in *err) if the setup
 * is outside what the stage handles — a book with more than 65536 entries, a vector length that does not divide the
 * partition size, more than 8192 (pass, partition, channel) slots per packet, a residue vector longer than 65535 or a
 * submap that can hold more than 65535 entry numbers in one pass; the caller then keeps feeding floats. */
int vsyn_attach_vq(vsyn_handle* h, const vsyn_vq_setup* vq, const char** err);

/* vsyn_submit_device / vsyn_submit_host with the residue given as VQ entries: `residue` becomes an OUTPUT of
 * residue_floats floats (same packing as the input of vsyn_submit_*: it is the "after_residue" tensor; device scratch
 * for vsyn_submit_device_vq, optional — may be NULL — copy-back for vsyn_submit_host_vq). Requires vsyn_attach_vq. */
int vsyn_submit_device_vq(vsyn_handle* h,
                          uint32_t num_packets, const vsyn_packet* d_packets,
                          uint32_t num_segments, const vsyn_segment* d_segments, uint32_t max_seg_packets,
                          const uint16_t* d_ys, const vsyn_vq_batch* d_vq, float* d_residue,
                          float* d_pcm, uint64_t plane_stride,
                          uint32_t* d_emit_len, const vsyn_taps* d_taps,
                          uint32_t flags, void* hip_stream, const char** err);
int vsyn_submit_host_vq(vsyn_handle* h,
                        uint32_t num_packets, const vsyn_packet* packets,
                        uint32_t num_segments, const vsyn_segment* segments,
                        const uint16_t* ys, const vsyn_vq_batch* vq, float* residue_out, size_t residue_floats,
                        float* pcm, uint64_t plane_stride,
                        uint32_t* emit_len, const vsyn_taps* taps,
                        uint32_t flags, vsyn_status* status, const char** err);

/* ---- PCM post-stage: planar f32 -> what the consumer of gotPcmData does next ----
 * Converts the PCM of the MOST RECENT vsyn_submit_device* call on this handle (stream-ordered: pass the same hip_stream)
 * from planar [S][channels][plane_stride] to interleaved frames [S][out_stride_frames][channels]; segment g gets its
 * total emitted frames (the sum of its emit_len), also written to d_frames[g] if d_frames != NULL.
 *   VSYN_PCM_S16  int16, host endian, val = round-to-nearest-even(x * 32768.f) clamped to [-32768, 32767] — ov_read's
 *                 conversion (reference tree: tests/libvorbis-standalone/vorbis_vorbisfile.c:2026-2029 with vorbis_ftoi of
 *                 os.h:156-158); halves the output bytes. +Inf and every product above 32767 give 32767, -Inf and every product
 *                 below -32768 give -32768, and a NaN gives -32768 (ov_read's own value: its conversion of a NaN is INT_MIN, which
 *                 the clamp cuts), at every site that writes int16: both forms of this entry, vsyn_pcm_fetch_host and
 *                 vsyn_pcm_resample_host
 *   VSYN_PCM_F32  float32, values unchanged */
#define VSYN_PCM_S16 1
#define VSYN_PCM_F32 2
int vsyn_pcm_interleave_device(vsyn_handle* h, int format, const float* d_pcm, uint64_t plane_stride,
                               void* d_out, uint64_t out_stride_frames, uint32_t* d_frames,
                               void* hip_stream, const char** err);

/* Per-(segment, channel) digest of the PCM of the MOST RECENT vsyn_submit_host / vsyn_submit_host_vq call on this handle:
 * out[g * channels + c] = sum of |x| over segment g's emitted frames of channel c, accumulated in double in a fixed order (the
 * same PCM always gives the same bits). Computed on the device from the PCM still resident there, so that a corpus decoder
 * can tell that replicas agree — the reference's harness compares decoders sample by sample, compare-debug-out.py:524-542 —
 * without another pass over the PCM on the host. `out` holds S * channels doubles of the last submit. Synchronous. */
int vsyn_pcm_abs_sum_host(vsyn_handle* h, double* out, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* call on this handle, converted on the device and copied to the host in the
 * interleaved form of vsyn_pcm_interleave_device (VSYN_PCM_S16 / VSYN_PCM_F32): out[g][frame][channel], out_stride_frames
 * frames per segment (frames past a segment's end are zero); frames_out[g] (optional) = emitted frames of segment g. With VSYN_SUBMIT_KEEP_PCM on the submit, int16
 * output halves the bytes that cross the bus. Synchronous. */
int vsyn_pcm_fetch_host(vsyn_handle* h, int format, void* out, uint64_t out_stride_frames, uint32_t* frames_out, const char** err);

/* Page-locked host memory for the buffers handed to vsyn_submit_host (direct DMA instead of the runtime's staging copies;
 * what a host decoder that batches at corpus scale wants). Pageable memory is accepted by vsyn_submit_host as well. */
int vsyn_host_alloc(size_t bytes, void** out, const char** err);
void vsyn_host_free(void* p);

/* Waits for hip_stream and returns the accumulated device status since the last call (then clears it). */
int vsyn_sync_status(vsyn_handle* h, void* hip_stream, vsyn_status* status, const char** err);

/* Forget all overlap state (every stream slot behaves as VSYN_SEG_RESET on its next segment). */
int vsyn_reset_streams(vsyn_handle* h, void* hip_stream, const char** err);

/* Kernel timing for roofline reporting: when enabled, vsyn_submit_device brackets its dominant kernel with
 * hipEvents on hip_stream; vsyn_profile_read synchronises and returns the mean duration since the last read. */
int vsyn_profile_enable(vsyn_handle* h, int on); /* 0 off, 1 or 2 time the fused synthesis kernel (one kernel serves steady and mixed-block runs), 3 the residue VQ kernel */
int vsyn_profile_read(vsyn_handle* h, double* mean_ms, uint32_t* launches, const char** kernel_name);

/* IMDCT-only entry (BASELINE config 2): in [count][n/2] -> out [count][n], device pointers, n = blocksize0 or blocksize1. */
int vsyn_imdct_device(vsyn_handle* h, uint32_t n, uint32_t count, const float* d_in, float* d_out,
                      void* hip_stream, const char** err);

/* ---- feature matrices: the reference's RETURNN features without synthesising PCM ----
 *
 * What returnn_import.py:74-115 (get_features_from_raw_bytes) computes: demo_live_extract.py read_floor_ys (262-416) and
 * read_residue_ys (418-505) applied to the decoder's hook stream, filtered by name as returnn_import.py:84-113 does. One
 * float32 row of output_dim columns per hook that makes a row, rows in hook order. The reference's quirks are the contract:
 *
 *  - Hook order per packet (hpp:1160-1211): for every channel c, "floor_number"; if c's floor is used (vsyn_packet.floor_used
 *    bit c, before the nonzero propagate), "floor1 final_ys" (hpp:560) and "floor1 floor" (hpp:585). After all channels,
 *    "after_residue" for EVERY channel, used floor or not. "floor1 final_ys" holds the posts BEFORE the multiplier (the
 *    reader multiplies); "floor1 floor" has n entries, its second half flat.
 *  - biggest floor = the first floor with the most posts.
 *  - Floor kinds: one row per (packet, channel) with a used floor, in that order; with VSYN_FEAT_ONLY_BIGGEST_FLOOR only for
 *    channels whose floor is the biggest (the floor-number column is then off). Column 0 (VSYN_FEAT_INCLUDE_FLOOR_NUMBER) is
 *    (f + 1) / num_floors - 0.5 computed in double and rounded to float. Values: v / 255 (VSYN_FEAT_FLOOR_ALWAYS_POSITIVE) or
 *    (v - 127.5) / 127.5 in float32, v = final_y * multiplier resp. the rendered curve gathered at xs; columns past the
 *    data are 0.
 *  - The rendered kind's xs: the floor's own xs (header order, ascending with VSYN_FEAT_SORTED_XS); with upscale_xs_factor
 *    != 1 those xs through scipy.ndimage.zoom(order=1, mode="nearest") and numpy.round (restated on the host; a factor whose
 *    output length is not len(xs) * factor fails like the reference's assert); with VSYN_FEAT_XS_FROM_BIGGEST_FLOOR the
 *    biggest floor's (upscaled) xs, for another floor f floor-divided by factor = round(max xs_big / max xs_f) (Python's
 *    round; 0 gives 0, as numpy does) and clipped to [0, n-1]. An unclipped index past the n entries fails the batch with
 *    VSYN_ST_FEATURE_INDEX (the reference raises IndexError), whether or not its column is kept.
 *  - Residue kinds: the reader's floor number at "after_residue" time is the LAST channel's: a packet gives one row per
 *    channel (zeros for channels without residue) exactly when channel C-1's floor is the biggest. Row = after_residue
 *    gathered at clip(xs_big[:output_dim], 0, n/2-1) (VSYN_FEAT_IGNORE_XS: bins 0..min(n/2, output_dim)-1); without
 *    VSYN_FEAT_IGNORE_XS an output_dim below the biggest floor's post count is refused (the reference asserts,
 *    demo_live_extract.py:484-485). VSYN_FEAT_RESIDUE_YS_WITH_FLOOR: floor_base = the most recent biggest-floor "floor1
 *    floor" of the segment (carried over packets without one; none before the first) gathered the same way at clip(., 0, n-1)
 *    and divided by 255; float32 order: log1p(|x|) (VSYN_FEAT_LOG1P_ABS_SPACE), then + floor_base * floor_base_factor resp.
 *    * exp((floor_base - 1) * floor_base_factor) (log1p, exp rounded once from double), then * scale, then clip to +-clip_abs_max (VSYN_FEAT_CLIP). With
 *    VSYN_FEAT_IGNORE_XS a floor_base whose length differs from the row's fails with VSYN_ST_FEATURE_INDEX (numpy cannot
 *    broadcast them).
 *  - The reference's floor_final_ys_rendered_concat_residue (scipy zoom order 3) is not provided.
 *  - A segment is a whole stream from its first audio packet: nothing carries across calls, and the features entry points
 *    neither read nor write the handle's overlap state or the PCM of the most recent submit. The checks are those of the
 *    reference that concern floors and packets: VSYN_ST_FLOOR_RANGE, VSYN_ST_FLOOR_VALUE (any of the n floor entries >= 256),
 *    VSYN_ST_BAD_MODE, VSYN_ST_BAD_SEGMENT, plus VSYN_ST_FEATURE_INDEX; a flagged batch's rows are unspecified.
 */
#define VSYN_ST_FEATURE_INDEX (1u << 8) /* feature entry points: a gather index past its vector, or floor_base / row lengths differ */

enum {
  VSYN_FEAT_FLOOR_FINAL_YS = 1,          /* kind "floor_final_ys" */
  VSYN_FEAT_FLOOR_FINAL_YS_RENDERED = 2, /* kind "floor_final_ys_rendered" */
  VSYN_FEAT_RESIDUE_YS = 3,              /* kind "residue_ys" */
  VSYN_FEAT_RESIDUE_YS_WITH_FLOOR = 4    /* kind "residue_ys_with_floor" */
};
/* vsyn_feature_spec.options */
#define VSYN_FEAT_INCLUDE_FLOOR_NUMBER 1u   /* floor kinds */
#define VSYN_FEAT_ONLY_BIGGEST_FLOOR 2u     /* floor kinds; excludes VSYN_FEAT_INCLUDE_FLOOR_NUMBER */
#define VSYN_FEAT_SORTED_XS 4u              /* all kinds */
#define VSYN_FEAT_XS_FROM_BIGGEST_FLOOR 8u  /* floor kinds */
#define VSYN_FEAT_FLOOR_ALWAYS_POSITIVE 16u /* floor kinds */
#define VSYN_FEAT_LOG1P_ABS_SPACE 32u       /* residue kinds */
#define VSYN_FEAT_IGNORE_XS 64u             /* residue kinds */
#define VSYN_FEAT_CLIP 128u                 /* residue kinds: clip_abs_max is set and > 0 */

typedef struct vsyn_feature_spec {
  uint32_t kind;               /* VSYN_FEAT_* kind */
  uint32_t output_dim;         /* columns per row, >= 1 */
  uint32_t options;            /* VSYN_FEAT_* option bits */
  uint32_t reserved0;
  double upscale_xs_factor;    /* rendered kind: 1 = off */
  float scale;                 /* residue kinds: 1 = off */
  float clip_abs_max;          /* residue kinds, with VSYN_FEAT_CLIP */
  float floor_base_factor;     /* residue_ys_with_floor: 1 = the reference's default */
  uint32_t reserved1;
} vsyn_feature_spec;

/* Device pointers, asynchronous on hip_stream. vsyn_feature_rows_device writes d_seg_row_off[S+1] (uint64): segment g's rows
 * are [d_seg_row_off[g], d_seg_row_off[g+1]). vsyn_features_device computes the same offsets (d_seg_row_off may be NULL) and
 * writes the rows, d_rows[d_seg_row_off[S]][output_dim]; d_residue may be NULL for the floor kinds. No IMDCT, no PCM.
 * max_seg_packets >= every segment's num_packets. Errors found on the device are reported by vsyn_sync_status. */
int vsyn_feature_rows_device(vsyn_handle* h, const vsyn_feature_spec* spec,
                             uint32_t num_packets, const vsyn_packet* d_packets,
                             uint32_t num_segments, const vsyn_segment* d_segments, uint32_t max_seg_packets,
                             uint64_t* d_seg_row_off, void* hip_stream, const char** err);
int vsyn_features_device(vsyn_handle* h, const vsyn_feature_spec* spec,
                         uint32_t num_packets, const vsyn_packet* d_packets,
                         uint32_t num_segments, const vsyn_segment* d_segments, uint32_t max_seg_packets,
                         const uint16_t* d_ys, const float* d_residue,
                         float* d_rows, uint64_t* d_seg_row_off, void* hip_stream, const char** err);
/* HOST pointers: stages, runs, copies back, synchronises. seg_rows[S] receives each segment's row count; rows (may be NULL
 * when only the counts are wanted) receives the rows of all segments back to back, at most rows_capacity rows (num_packets *
 * channels always suffices; VSYN_ERR_INVALID with the counts filled if it is too small). VSYN_ERR_STREAM if flagged. */
int vsyn_features_host(vsyn_handle* h, const vsyn_feature_spec* spec,
                       uint32_t num_packets, const vsyn_packet* packets,
                       uint32_t num_segments, const vsyn_segment* segments,
                       const uint16_t* ys, const float* residue, size_t residue_floats,
                       float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                       vsyn_status* status, const char** err);

/* ---- spectral features: mel filterbank, log-mel, dB-mel and MFCC of the decoded PCM, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames (what ogg_vorbis_decode_corpus returns per file).
 * Output: a float32 matrix (frames, dim), time-major like the feature matrices. The math follows librosa's documented defaults
 * (librosa >= 0.10); it is written below as exact arithmetic, and the device is compared against a float64 model of it
 * (tests/spectral_model.py). Parity with librosa itself has NOT been verified (librosa is not among the test dependencies).
 *
 *  1. Mono: y[t] = (1/C) * sum_c x[c][t]                                                     (librosa.to_mono)
 *  2. Framing: VSYN_SPEC_CENTER pads n_fft/2 zeros on both sides; T_pad = T (+ 2 * (n_fft/2)). Frames
 *     F = 1 + (T_pad - n_fft) / hop_length if T_pad >= n_fft, else 0; F = 0 whenever T = 0. Frame f starts at padded index
 *     f * hop_length (vsyn_spectral_num_frames).
 *  3. Window: periodic Hann of win_length, w[i] = 0.5 - 0.5 cos(2 pi i / win_length), zero-padded centred to n_fft at offset
 *     (n_fft - win_length) / 2.
 *  4. S[f][k] = |sum_j w[j] y_pad[f*hop + j] exp(-2 pi i j k / n_fft)|^power, k = 0 .. n_fft/2, power 1 or 2. Any n_fft in
 *     [16, 8192], powers of two or not (int(0.025 * 44100) = 1102 is the usual 25 ms window).
 *  5. Mel filterbank (librosa.filters.mel): bin frequencies k * sr / n_fft; n_mels + 2 edges equally spaced in mel between
 *     mel(fmin) and mel(fmax) (fmax = 0: sr/2; fmax > sr/2 refused), mapped back to Hz: hz[0 .. n_mels+1]. Slaney mel scale:
 *     f / (200/3) below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27) above; VSYN_SPEC_HTK: 2595 log10(1 + f / 700).
 *     W[m][k] = max(0, min((f_k - hz[m]) / (hz[m+1] - hz[m]), (hz[m+2] - f_k) / (hz[m+2] - hz[m+1]))), times
 *     2 / (hz[m+2] - hz[m]) (Slaney area normalisation; VSYN_SPEC_NO_NORM turns it off). M[f][m] = sum_k W[m][k] S[f][k].
 *     The table is built in double on the host, per distinct sample rate.
 *  6. Kinds: VSYN_SPEC_MEL_POWER = M. VSYN_SPEC_LOG_MEL = log10(max(M, log_floor)) (RETURNN's log filterbank).
 *     VSYN_SPEC_MEL_DB = librosa power_to_db(ref=1): D = 10 log10(max(M, amin)), then if top_db > 0,
 *     D = max(D, max over the whole segment of D - top_db). VSYN_SPEC_MFCC = the orthonormal DCT-II of MEL_DB along the mel
 *     axis, first n_mfcc coefficients (librosa.feature.mfcc, lifter 0). dim = n_mfcc for MFCC, n_mels otherwise.
 *  7. Checks (VSYN_ERR_INVALID before anything runs): 1 <= hop_length; 1 <= win_length <= n_fft; 16 <= n_fft <= 8192;
 *     1 <= n_mels <= 256; 1 <= n_mfcc <= n_mels (MFCC); 0 <= fmin < fmax <= sr/2 for every segment's rate; power 1 or 2;
 *     log_floor > 0 (LOG_MEL); amin > 0 and top_db >= 0 (MEL_DB, MFCC).
 *  8. Not finite. Nothing is refused and no status is raised. Frame f reads the samples of its window's support alone, PCM frames
 *     [f hop - pad + woff, f hop - pad + woff + win_length), pad = n_fft / 2 with VSYN_SPEC_CENTER else 0,
 *     woff = (n_fft - win_length) / 2. If one of them is Inf or NaN in any channel (under a window value of zero as well), every
 *     value of row f is Inf or NaN, for every kind: the floors of step 6 keep a NaN (max(NaN, floor) is NaN here, as numpy.maximum
 *     has it). Every other row has the bits it has without that sample, with one exception that is a rule of its own: with
 *     top_db > 0 the segment's maximum is taken over its finite D values only, so a value that is not finite takes no part in it,
 *     and the clamp leaves such a value as it is. Rows outside the footprint are therefore clamped against the maximum of the
 *     finite values, and a segment without a finite value is not clamped. Samples behind a segment's frames, or that no
 *     frame's support holds, are never read. Other segments are not touched.
 *
 * Precision: windowed samples, twiddles cos/sin(2 pi m / n_fft) (rounded from double) and mel weights are float32; the DFT
 * and the mel sums accumulate in float32 in a fixed order, so the same PCM always gives the same bits. The error of the DFT
 * chain grows with n_fft (DESIGN.md "Spectral features": at 8192 the log kinds lose digits on low, near-silent bands). The spectral entry
 * points read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM, and a
 * later vsyn_pcm_fetch_host returns the same PCM. One handle's spectral entry points share its spectral workspace. */
enum {
  VSYN_SPEC_MEL_POWER = 1,  /* "mel_power" */
  VSYN_SPEC_LOG_MEL = 2,    /* "log_mel" */
  VSYN_SPEC_MEL_DB = 3,     /* "mel_db" */
  VSYN_SPEC_MFCC = 4        /* "mfcc" */
};
/* vsyn_spectral_spec.options */
#define VSYN_SPEC_CENTER 1u   /* pad n_fft/2 zeros on both sides (librosa's center=True) */
#define VSYN_SPEC_HTK 2u      /* HTK mel scale instead of Slaney's */
#define VSYN_SPEC_NO_NORM 4u  /* no Slaney area normalisation of the filters */

typedef struct vsyn_spectral_spec {
  uint32_t kind;        /* VSYN_SPEC_* kind */
  uint32_t options;     /* VSYN_SPEC_* option bits */
  uint32_t n_fft, hop_length, win_length, n_mels;  /* n_mels: the mel kinds only */
  uint32_t n_mfcc;      /* MFCC only */
  uint32_t power;       /* 1 (magnitude) or 2 (power) */
  double fmin, fmax;    /* Hz; fmax = 0: each segment's sr / 2 */
  double log_floor;     /* LOG_MEL */
  double amin, top_db;  /* MEL_DB, MFCC, LIN_DB; top_db = 0: no clamp */
} vsyn_spectral_spec;

/* Frames of a segment of `frames` PCM frames under spec (step 2), 0 for an invalid spec. */
uint64_t vsyn_spectral_num_frames(const vsyn_spectral_spec* spec, uint64_t frames);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle (with or without VSYN_SUBMIT_KEEP_PCM), per segment of that
 * submit. sample_rates[S] (host) is each segment's rate; a rate of 0 skips the segment (0 rows). seg_rows[S] receives each
 * segment's row count; rows (may be NULL when only the counts are wanted) receives the rows of all segments back to back, dim
 * columns each, at most rows_capacity rows (VSYN_ERR_INVALID with the counts filled if it is too small). status as for
 * vsyn_features_host. Synchronous. */
int vsyn_pcm_spectral_host(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                           float* rows, uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status, const char** err);
/* The caller's planar PCM: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) PCM frames per segment (clamped to
 * plane_stride). sample_rates[S] is a HOST array as above. Writes d_seg_row_off[S+1] (uint64, may be NULL): segment g's rows
 * are [d_seg_row_off[g], d_seg_row_off[g+1]) of d_rows, which must hold sum_g vsyn_spectral_num_frames(spec, frames_g) rows of
 * dim columns (S * vsyn_spectral_num_frames(spec, plane_stride) always suffices). Asynchronous on hip_stream. */
int vsyn_spectral_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                         const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames,
                         float* d_rows, uint64_t* d_seg_row_off, void* hip_stream, const char** err);

/* ---- linear spectra: magnitude / power, their dB image and the complex STFT of the decoded PCM, computed where the PCM is ----
 *
 * Three more kinds of vsyn_spectral_spec, served by every spectral entry point above and below (vsyn_spectral_device, the
 * vsyn_pcm_*spectral*_host forms, the corpus runs): the linear-frequency spectrum that the mel kinds are built from, without a
 * filterbank. Input, output layout and frame count are those of "spectral features"; the device is compared against a float64
 * model of the arithmetic below (tests/spectral_lin_model.py) under a per-frame error bound.
 *
 *  1. Mono, framing and window: steps 1 - 3 of "spectral features", unchanged. vsyn_spectral_num_frames gives F; row f lines up
 *     with row f of the mel kinds, of the pitch frames and of the frame descriptors at the same n_fft, hop and centring.
 *  2. v[j] = w[j] * y_pad[f * hop_length + j], j < n_fft (0 outside the window's support), and
 *     X[k] = sum_j v[j] exp(-2 pi i j k / n_fft), k = 0 .. NB - 1, NB = n_fft / 2 + 1.
 *  3. Kinds. VSYN_SPEC_LIN_POWER: S[k] = |X[k]|^power, power 1 or 2; dim = NB.
 *     VSYN_SPEC_LIN_DB: D[k] = 10 log10(max(S[k], amin)), then if top_db > 0, D = max(D, max over the whole segment of D - top_db):
 *     step 6's MEL_DB with S in M's place; dim = NB. librosa.amplitude_to_db(|X|, amin=a) is this kind with power = 2, amin = a^2.
 *     VSYN_SPEC_STFT: re_0, im_0, re_1, im_1, ... with re_k = sum_j v[j] cos(2 pi j k / n_fft), im_k = -sum_j v[j] sin(2 pi j k /
 *     n_fft) (numpy.fft.rfft's sign); dim = 2 NB; power, amin and top_db are not read.
 *  4. Not read by these kinds, and not checked: n_mels, n_mfcc, fmin, fmax, VSYN_SPEC_HTK, VSYN_SPEC_NO_NORM, log_floor. A
 *     segment's rate only decides whether it is skipped (rate 0: 0 rows); no mel table is built. Checked (VSYN_ERR_INVALID before
 *     anything runs): the option bits, n_fft, hop_length, win_length as in step 7 there; power 1 or 2 (LIN_POWER, LIN_DB); amin > 0
 *     and top_db >= 0 (LIN_DB).
 *  5. The post stage ("spectral post-processing") holds rows of at most 256 columns and is refused for these kinds: every entry
 *     point given a vsyn_spectral_post with the stage on (order != 0 or a normalisation) returns VSYN_ERR_INVALID before anything
 *     runs, and vsyn_spectral_post_dim returns 0. A post spec with the stage off is accepted and does nothing, as for the mel kinds.
 *  6. Inf and NaN samples: step 8 of "spectral features", word for word, with S in M's place for LIN_DB (the amin floor keeps a
 *     NaN; the segment's maximum is over its finite D values; the clamp leaves a value that is not finite as it is). A frame whose
 *     window's support holds such a sample is Inf / NaN in every bin, other frames are not touched, nothing is refused. For
 *     VSYN_SPEC_STFT a value is the complex bin: at least one of re_k, im_k is Inf or NaN (im_0 and, for an even n_fft, the last
 *     bin's im may be the 0 that a real transform gives them, as in numpy.fft.rfft).
 *
 * Arithmetic: float32 throughout, in a fixed order per frame, so that the same PCM gives the same bits alone, in any slot of a
 * batch, at any alignment of the plane and wherever the frame falls in its workgroup's tile. n_fft a power of two: v[j] is one
 * rounded product, then a real-input radix-2 FFT per frame (a half-size complex transform of the even and odd samples and an
 * untangling pass) with the twiddles cos/sin(2 pi m / n_fft) rounded from double; each of re_k, im_k is within
 * 4 (log2 n_fft + 2) 2^-24 sum_j |v[j]| of the exact sum. Any other n_fft: the direct sum of "spectral features", one fma chain
 * per component, j ascending over the window's support; within (win_length + 3) 2^-24 sum_j |v[j]|. A row of these kinds has up to
 * 8194 floats: size rows buffers by vsyn_spectral_dim. */
enum {
  VSYN_SPEC_LIN_POWER = 5,  /* "lin_power" */
  VSYN_SPEC_LIN_DB = 6,     /* "lin_db" */
  VSYN_SPEC_STFT = 7        /* "stft" */
};

/* Columns of a row under spec (n_mels; n_mfcc for MFCC; NB for LIN_POWER and LIN_DB; 2 NB for STFT), 0 for an invalid spec and for
 * the kinds of "chroma" below (vsyn_spectral_chroma_dim answers for those). */
uint32_t vsyn_spectral_dim(const vsyn_spectral_spec* spec);
/* Frames that one workgroup of the linear kinds' kernel computes under spec (a tuning fact, exposed for tests that place frame
 * counts around it); 0 for an invalid spec or a mel kind. */
uint32_t vsyn_spectral_lin_tile(const vsyn_spectral_spec* spec);

/* ---- chroma: pitch-class rows (librosa.feature.chroma_stft) and the tonnetz rows computed from them, where the PCM is ----
 *
 * Two more kinds of vsyn_spectral_spec, served by every spectral entry point above and below with the default chroma parameters,
 * and by the entry points of this section with a vsyn_spectral_chroma of the caller's (vsyn_spectral_dim alone still answers 0 for
 * them: vsyn_spectral_chroma_dim sizes their rows). librosa is not among the test dependencies
 * and parity with it is not claimed: the contract is the exact arithmetic below, and the device is compared against a float64
 * model of it (tests/chroma_model.py) under a per-frame error bound.
 *
 *  1. Mono, framing, window and X[k]: steps 1 - 3 of "spectral features" and step 2 of "linear spectra", unchanged.
 *     S[k] = |X[k]|^power, power 1 or 2 (chroma_stft's is 2), k < NB = n_fft / 2 + 1. Row f lines up with row f of every other kind
 *     at the same n_fft, hop and centring.
 *  2. Filterbank (librosa.filters.chroma with its inner norm = 2), built in double on the host, once per distinct sample rate sr:
 *       fr[j] = j sr / n_fft, j = 1 .. n_fft - 1;  A = 440 * 2^(tuning / n_chroma);  q[j] = n_chroma log2(fr[j] / (A / 16));
 *       q[0] = q[1] - 1.5 n_chroma;  bw[j] = max(q[j+1] - q[j], 1) for j < n_fft - 1, bw[n_fft-1] = 1;
 *       h = rint(n_chroma / 2) with ties to even (numpy.round);  D[c][j] = mod(q[j] - c + h + 10 n_chroma, n_chroma) - h with a
 *       non-negative mod;  W[c][j] = exp(-0.5 (2 D[c][j] / bw[j])^2).
 *     Every column j is divided by its L2 norm over c (a norm below DBL_MIN counts as 1); unless VSYN_CHROMA_NO_OCT it is then
 *     multiplied by exp(-0.5 ((q[j] / n_chroma - ctroct) / octwidth)^2); with VSYN_CHROMA_BASE_C the rows are rotated so that new
 *     row c is old row (c + 3 (n_chroma / 12)) mod n_chroma (integer division): row 0 is C instead of A. Columns 0 .. NB - 1 are
 *     kept and cast to float32; a value whose magnitude is below FLT_MIN is stored as 0, so no weight is denormal.
 *     vsyn_chroma_filterbank returns this table.
 *  3. VSYN_SPEC_CHROMA: R[c] = sum_k W[c][k] S[k]; N = the norm of R over c chosen by vsyn_spectral_chroma.norm (L1: sum |R|, L2:
 *     sqrt(sum R^2), max: max |R|). The row is R[c] / N, or R itself when N < FLT_MIN (librosa.util.normalize's fill = None) and
 *     with norm none. dim = n_chroma.
 *  4. VSYN_SPEC_TONNETZ (librosa.feature.tonnetz(chroma = the rows of step 3)): u = the chroma row after its own norm, L1-normalised
 *     again with the same FLT_MIN rule; out[i] = sum_c phi[i][c] u[c], i < 6, phi[i][c] = r_i cos(pi (s_i 12 c / n_chroma - o_i)),
 *     s = (7/6, 7/6, 3/2, 3/2, 2/3, 2/3), o = (1/2, 0, 1/2, 0, 1/2, 0), r = (1, 1, 1, 1, 1/2, 1/2); phi is built in double on the
 *     host and rounded to float32. dim = 6.
 *  5. If any R[c] of a frame is not finite (an Inf or NaN sample inside the frame, or an overflow), every value of that frame's
 *     row is NaN, for both kinds and every norm; other frames are not touched.
 *  6. Checked (VSYN_ERR_INVALID before anything runs): the option bits, n_fft, hop_length, win_length and power as for "linear
 *     spectra"; 1 <= n_chroma <= 256; norm in 0 .. 3; no unknown chroma option bits; tuning and ctroct finite; octwidth finite and
 *     > 0 unless VSYN_CHROMA_NO_OCT. Not read and not checked: the mel fields, amin, top_db, log_floor. A rate of 0 skips its
 *     segment. tuning is a number here: the estimate that librosa's tuning = None runs first is a stage of its own ("tuning
 *     estimation"), which vsyn_pcm_chain_chroma_est_host runs in front of the filterbank per segment and a caller of the
 *     asynchronous entry chains in front himself (vsyn_tuning_device).
 *  7. PCEN is refused for both kinds. The post stage ("spectral post-processing") is accepted for both: their rows are at most 256
 *     columns wide.
 *
 * Arithmetic: float32 in a fixed order, so that the same PCM gives the same bits alone, in any slot of a batch, at any alignment of
 * the plane and wherever the frame falls in its workgroup's tile. n_fft a power of two: the FFT of "linear spectra", S[k] kept in
 * LDS; R[c] by one wave per (frame, c): lane l runs one fma chain over k = l, l + 64, ... ascending, then the 64 partial sums are
 * added in an xor-shuffle tree (lane distance 32, 16, 8, 4, 2, 1). Any other n_fft: the direct sum of "spectral features" in chunks
 * of 256 bins; per chunk the same chain and tree over the chunk's bins, the chunks' sums added to R[c] in ascending order. The norm's
 * sum (L1: |R|, L2: (R / m)^2, max) runs per frame in one wave: lane l over c = l, l + 64, ... ascending, then the same tree; L2 is
 * m sqrtf(sum (R / m)^2) with m = max |R| (and N = m when m < FLT_MIN), so that the squares neither overflow nor vanish. Tonnetz: the second L1 sum likewise, then one fma chain per i over c ascending. The linear rows never
 * leave the workgroup. */
enum {
  VSYN_SPEC_CHROMA = 8,  /* "chroma" */
  VSYN_SPEC_TONNETZ = 9  /* "tonnetz" */
};
/* vsyn_spectral_chroma.norm */
enum { VSYN_CHROMA_NORM_NONE = 0, VSYN_CHROMA_NORM_L1 = 1, VSYN_CHROMA_NORM_L2 = 2, VSYN_CHROMA_NORM_MAX = 3 };
/* vsyn_spectral_chroma.options */
#define VSYN_CHROMA_BASE_C 1u  /* row 0 is pitch class C (librosa's base_c=True); without it, A */
#define VSYN_CHROMA_NO_OCT 2u  /* no Gaussian octave weighting (librosa's octwidth=None); ctroct and octwidth are not read */

typedef struct vsyn_spectral_chroma {
  uint32_t n_chroma;  /* 1 .. 256 */
  uint32_t norm;      /* VSYN_CHROMA_NORM_* */
  uint32_t options;   /* VSYN_CHROMA_* option bits */
  uint32_t reserved;  /* 0 */
  double tuning;      /* deviation from A440 in fractions of a chroma bin */
  double ctroct, octwidth;  /* centre and width of the octave weighting, in octaves (units of q / n_chroma) */
} vsyn_spectral_chroma;
/* The defaults, which a NULL vsyn_spectral_chroma means everywhere: {12, VSYN_CHROMA_NORM_MAX, VSYN_CHROMA_BASE_C, 0, 0.0, 5.0, 2.0}. */

/* The columns of a row of every kind. vsyn_spectral_dim predates the chroma kinds and keeps answering 0 for kinds 8 and 9, as it did
 * when they were unknown: a row's width is a chroma parameter, which it does not take. Size rows buffers of these kinds with this
 * function. With the chroma parameters (NULL: the defaults): n_chroma for CHROMA, 6 for TONNETZ, vsyn_spectral_dim(spec) for
 * every other kind (chroma is then neither read nor checked); 0 for an invalid spec or chroma. */
uint32_t vsyn_spectral_chroma_dim(const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma);
/* The float32 filterbank of step 2 at sample_rate, as the device gets it: out[c * NB + k], n_chroma rows of NB = n_fft / 2 + 1. Host
 * only: no device is needed. VSYN_ERR_INVALID for a NULL out, sample_rate 0, or a spec / chroma that step 6 refuses (spec->kind must
 * be CHROMA or TONNETZ). */
int vsyn_chroma_filterbank(uint32_t sample_rate, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma, float* out);
/* Frames that one workgroup of the chroma kernels computes under spec (a tuning fact, exposed for tests that place frame counts
 * around it); 0 for an invalid spec or another kind. */
uint32_t vsyn_spectral_chroma_tile(const vsyn_spectral_spec* spec);
/* vsyn_spectral_device with the chroma parameters (NULL: the defaults; with a kind other than CHROMA and TONNETZ chroma is not read and
 * the call is vsyn_spectral_device). */
int vsyn_spectral_chroma_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma, uint32_t num_segments,
                                const uint32_t* sample_rates, const float* d_pcm, uint64_t plane_stride, uint32_t channels,
                                const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off, void* hip_stream, const char** err);

/* ---- tuning estimation: spectral peaks (librosa.piptrack) and the tuning taken from them (librosa.estimate_tuning), where the PCM is ----
 *
 * librosa is not among the test dependencies and parity with it is not claimed: the contract is the arithmetic below and a float64
 * model of it (tests/tuning_model.py). The result is the number that vsyn_spectral_chroma.tuning (with n_chroma = bins_per_octave)
 * and vsyn_cqt_spec.tuning take: a deviation from A440 in fractions of a bin of bins_per_octave.
 *
 *  1. Spectrum. Per segment and frame f, S[k], k < NB = n_fft / 2 + 1, is the float32 value of VSYN_SPEC_LIN_POWER ("linear
 *     spectra") at the same n_fft, hop_length, win_length, centring and power (1 or 2), bit for bit. It stays in LDS.
 *  2. Searched bins, on the host in double, per distinct rate sr: fmin' = max(fmin, 0), fmax' = min(fmax, sr / 2); [k_lo, k_hi) holds
 *     the bins k < NB with fmin' <= k sr / n_fft < fmax' (vsyn_piptrack_bins; k_lo = k_hi = 0 when there is none).
 *  3. Peaks, in float32 unless stated. ref = threshold32 * max_k S[k], the maximum over all NB bins and threshold32 the threshold
 *     rounded to float32; Z[k] = S[k] > ref ? S[k] : 0. Bin k is a peak when k_lo <= k < k_hi, Z[k] > Z[k-1] and Z[k] >= Z[k+1], with
 *     replicated edges Z[-1] = Z[0], Z[NB] = Z[NB-1]: bin 0 is never a peak, the last bin can be one.
 *  4. Interpolation at a peak. For 1 <= k <= NB - 2: a = 0.5f * (S[k+1] - S[k-1]), b = (2 S[k] - S[k+1]) - S[k-1], and b = b + 1 if
 *     |b| < FLT_MIN; s = a / b. At k = 0 and k = NB - 1, a = s = 0. pitch = float32(((double)k + (double)s) * ((double)sr / n_fft)),
 *     mag = S[k] + (0.5f * a) * s. Every bin that is no peak holds 0 in both outputs. The library is built without fused contraction.
 *  5. A frame with any S[k] that is not finite (an Inf or NaN sample inside it, or an overflow) has NaN in every value of both its
 *     rows and contributes no peak to the tuning; other frames are not touched.
 *  6. Tuning, per segment over all its frames. P = the entries with pitch > 0, n = |P|. n = 0: the tuning is 0.0. Else the threshold
 *     is the median of mag over P: n odd, the middle element of the ascending float32 order; n even, (lo + hi) / 2 of the two middle
 *     ones rounded in float32 (numpy.median of a float32 array). Selected are the entries of P with mag >= threshold.
 *  7. Residual of a selected entry, in double: r = fmod(bins_per_octave * log2((double)pitch / 27.5), 1.0), and r = r - 1 if r >= 0.5.
 *     librosa takes this residual in float32; double is chosen here because every platform's double log2 agrees to an ulp or two,
 *     which the histogram's edges absorb, while a float32 chain would tie the result to one libm. fmod keeps the sign of its first
 *     argument: a pitch below 27.5 Hz can give r < -0.5, and such an entry is selected and counted nowhere.
 *  8. Histogram. nbin = ceil(1 / resolution); edges e_i = -0.5 + i * (1.0 / nbin), i = 0 .. nbin, built on the host in double. An entry
 *     counts in the bin i with e_i <= r < e_{i+1}: floor((r + 0.5) nbin), corrected by at most one against the table. The tuning is e_i
 *     of the FIRST bin with the largest count, a double. counts = {n, number selected}.
 *  9. Checked (VSYN_ERR_INVALID before anything runs): the spectral spec as for "linear spectra", and its kind must be
 *     VSYN_SPEC_LIN_POWER (power 1 or 2); fmin and fmax finite with fmax > fmin'; threshold finite and >= 0; resolution finite with
 *     0 < resolution < 1 and nbin <= 4096; 1 <= bins_per_octave <= 256; reserved 0. A call in which a segment could hold more than
 *     2^31 peaks (frames times half the searched bins) is refused. A rate of 0 skips its segment: no rows, tuning 0.0, counts 0.
 *
 * Arithmetic: no floating-point atomics anywhere. One wave per frame takes the maximum in an xor-shuffle tree and walks the bins 64
 * at a time in ascending order, one lane per bin; a frame's peaks are compacted in ascending k by ballot and prefix count into the
 * frame's own run of the workspace. The median is an exact selection on the float32 bit patterns by integer counting (8 bits a pass),
 * the histogram's counts are integers. The same PCM gives the same bits alone, in any slot of a batch and wherever a frame falls in
 * its workgroup's tile.
 *
 * Workspace: the entries of this section use the handle's spectral table and frame counts, as every spectral and chroma entry does:
 * calls of these entries on one handle must be ordered on one stream (or by the caller) among themselves and with those. The peak
 * records are sized from plane_stride (frames it could hold times cap), not from the segments' actual lengths, and a call that
 * needs more room than the last frees and allocates, which waits for the device.
 *
 * In front of the pitch-class features: vsyn_pcm_chain_chroma_est_host ("chroma") and vsyn_pcm_cqt_est_host ("constant-Q") run the
 * estimate per segment and build their tables per (rate, tuning) pair. Deliberately not built: piptrack's ref callable (ref is
 * always threshold * the frame's maximum); windows other than Hann; librosa's float32 residual (step 7); the estimate inside the
 * asynchronous vsyn_spectral_chroma_device and vsyn_cqt_device, which keep taking a number: the tables are built on the host from
 * numbers the device has yet to compute, so a caller chains vsyn_tuning_device in front and passes each tuning on. */
#define VSYN_TUNING_ONLY 0u /* vsyn_pcm_tuning_host: the tuning and the counts */
#define VSYN_TUNING_ROWS 1u /* ... and the dense piptrack rows */

typedef struct vsyn_tuning_spec { /* 40 bytes */
  double fmin, fmax;        /* the searched band in Hz (librosa: 150, 4000) */
  double threshold;         /* of the frame's maximum (librosa: 0.1) */
  double resolution;        /* the histogram's bin width in fractions of a bin (librosa: 0.01) */
  uint32_t bins_per_octave; /* 1 .. 256 (librosa: 12) */
  uint32_t reserved;        /* 0 */
} vsyn_tuning_spec;

/* Host only, no device and no handle: step 9 on (spec, tun), VSYN_OK or VSYN_ERR_INVALID with *err (may be NULL) naming the refusal. */
int vsyn_tuning_check(const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, const char** err);
/* Host only: out = {k_lo, k_hi} of step 2 at sample_rate. VSYN_ERR_INVALID for a NULL out, a rate of 0 or what step 9 refuses. */
int vsyn_piptrack_bins(uint32_t sample_rate, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t out[2]);
/* Host only: steps 6 to 8 on host arrays freqs[n] and mags[n] (librosa.pitch_tuning behind estimate_tuning's median threshold). With
 * mags NULL every entry with freqs > 0 is selected, which is plain pitch_tuning. *tuning and counts = {n of step 6, selected} are
 * written. VSYN_ERR_INVALID (nothing written) for a NULL output, a resolution or bins_per_octave that step 9 refuses, or more than
 * 2^31 entries with freqs > 0. */
int vsyn_pitch_tuning(const float* freqs, const float* mags, uint64_t n, double resolution, uint32_t bins_per_octave, double* tuning,
                      uint64_t counts[2]);
/* Frames that one workgroup of the piptrack kernels computes under spec (a tuning fact, exposed for tests that place frame counts
 * around it); 0 for an invalid spec or a kind other than VSYN_SPEC_LIN_POWER. */
uint32_t vsyn_piptrack_tile(const vsyn_spectral_spec* spec);
/* The caller's planar PCM, as for vsyn_spectral_device. vsyn_piptrack_device writes d_seg_row_off[S+1] (uint64, may be NULL) and the
 * dense rows of steps 3 to 5 into d_pitches and d_mags, each sum_g vsyn_spectral_num_frames(spec, frames_g) rows of NB float32.
 * vsyn_tuning_device writes d_tuning[S] (double) and d_counts[S][2] (uint64: n, selected) of steps 6 to 8; the peaks go through the
 * handle's workspace, never through dense rows. Both asynchronous on hip_stream. */
int vsyn_piptrack_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t num_segments,
                         const uint32_t* sample_rates, const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames,
                         float* d_pitches, float* d_mags, uint64_t* d_seg_row_off, void* hip_stream, const char** err);
int vsyn_tuning_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t num_segments,
                       const uint32_t* sample_rates, const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames,
                       double* d_tuning, uint64_t* d_counts, void* hip_stream, const char** err);
/* The PCM of the MOST RECENT vsyn_submit_host* on this handle, as for vsyn_pcm_cqt_host: each segment resampled from in_rates[g] to
 * out_rate first when out_rate != 0. seg_rows[S] always receives each segment's frame count. what = VSYN_TUNING_ONLY: tuning[S] and
 * counts[S][2] (counts may be NULL); with a NULL tuning nothing is launched. what = VSYN_TUNING_ROWS: the dense rows of all segments
 * back to back into rows, 2 NB float32 a row (its NB pitches, then its NB magnitudes), at most rows_capacity rows (VSYN_ERR_INVALID
 * with seg_rows filled if that is too small; with a NULL rows nothing is launched), and the tuning as well where tuning is not NULL.
 * status as for vsyn_pcm_spectral_host. Synchronous. */
int vsyn_pcm_tuning_host(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t num_segments,
                         const uint32_t* in_rates, uint32_t out_rate, uint32_t what, double* tuning, uint64_t* counts, float* rows,
                         uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status, const char** err);

/* ---- resampling: polyphase resampling of the decoded PCM to a target sample rate, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, at rate r_in. Output: the same layout at rate r_out.
 * The arithmetic is scipy.signal.resample_poly(x, up, down) with its defaults (window ('kaiser', 5.0), padtype 'constant'),
 * which is also librosa's res_type="polyphase". It is NOT soxr (librosa's default res_type); parity with soxr is not a goal.
 * The device is compared against a float64 model of the arithmetic below (tests/resample_model.py).
 *
 *  1. Ratio: g = gcd(r_in, r_out), up = r_out / g, down = r_in / g. If up == down the output is the input, bit for bit.
 *  2. Filter: M = max(up, down), H = 10 M, N = 2 H + 1. For n in [0, N), m = n - H:
 *       h[n] = up * w[n] * sinc(m / M) / S,   sinc(x) = sin(pi x) / (pi x), sinc(0) = 1,
 *       w[n] = I0(5 sqrt(1 - (2 n / (N - 1) - 1)^2)) / I0(5)   (the symmetric Kaiser window, beta 5),
 *       S    = sum_n w[n] sinc(m / M)                          (firwin's DC normalisation).
 *     Built in double on the host, per distinct (r_in, r_out) pair, and rounded to float32.
 *  3. Output: T_out = ceil(T * up / down) frames (vsyn_resample_num_frames), and
 *       y[j] = sum_i x[i] h[j down - i up + H],   h = 0 outside [0, N), x = 0 outside [0, T)  (scipy's padtype 'constant').
 *     Polyphase form, as the device computes it: c = j down + H, phi = c mod up, i0 = c div up, K = ceil(N / up),
 *       y[j] = sum_{t < K4} P[phi][t] x[i0 - t],   P[phi][t] = h[phi + t up],   K4 = K rounded up to a multiple of 4.
 *     The taps with phi + t up >= N, those in [K, K4) among them, are +0: on finite input they add nothing and the sum is the one
 *     over t < K. They are read all the same, so the rule for Inf and NaN is by K4: output j of a channel is Inf or NaN exactly
 *     when one of x[i0 - K4 + 1 .. i0] of that channel, inside [0, T), is (0 * Inf and 0 * NaN are NaN), and has the bits it has
 *     without that sample otherwise. Nothing is refused; the other channel, other segments and T_out are not touched, and
 *     samples behind a segment's T frames are never read. The rule is the same whether a pair's table is kept in LDS or not.
 *  4. Per segment, per channel: each segment is resampled on its own, zero-padded at both ends; nothing carries across submits.
 *  5. Limits (VSYN_ERR_INVALID before anything runs): 1 <= r_in, 1 <= r_out, and the reduced M = max(up, down) <= 65536.
 *
 * Precision: the taps are float32; every output is one float32 FMA chain over t = 0, 1, ... in that order, so the same input
 * always gives the same bits. The resample entry points read PCM only: they touch neither stream state, the overlap buffers nor
 * the PCM kept by VSYN_SUBMIT_KEEP_PCM, and a later vsyn_pcm_fetch_host returns the same PCM. One handle's resample entry points
 * share its resample workspace. */
#define VSYN_RESAMPLE_MAX_M 65536u

/* T_out for `frames` input frames (step 3), 0 for an invalid pair (step 5). */
uint64_t vsyn_resample_num_frames(uint32_t r_in, uint32_t r_out, uint64_t frames);

/* The caller's planar PCM: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) input frames per segment (clamped
 * to plane_stride). in_rates[S] is a HOST array of each segment's rate; a rate of 0 skips the segment (0 output frames). Writes
 * d_out[(g * channels + c) * out_plane_stride + j] for j < T_out(g), and d_out_frames[S] (device) = T_out(g). out_plane_stride
 * must be at least vsyn_resample_num_frames(in_rates[g], out_rate, plane_stride) for every resampled segment, and below 2^32.
 * d_out and d_out_frames are in the input form of vsyn_spectral_device (sample rate out_rate). Asynchronous on hip_stream. */
int vsyn_resample_device(vsyn_handle* h, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, const float* d_pcm,
                         uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride,
                         uint32_t* d_out_frames, void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle (with or without VSYN_SUBMIT_KEEP_PCM), resampled per segment
 * from in_rates[S] (host; 0 skips the segment) to out_rate and copied to the host. frames_out[S] (host) receives each
 * segment's T_out. out (may be NULL when only the counts are wanted) receives, with out_stride_frames frames per segment:
 *   VSYN_PCM_F32  float32 PLANAR, out[(g * channels + c) * out_stride_frames + j]
 *   VSYN_PCM_S16  int16 interleaved, out[(g * out_stride_frames + j) * channels + c], converted as vsyn_pcm_interleave_device does
 * Frames past a segment's T_out are zero. An out_stride_frames below some segment's T_out is VSYN_ERR_INVALID, with frames_out
 * filled. Synchronous. */
int vsyn_pcm_resample_host(vsyn_handle* h, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, int format, void* out,
                           uint64_t out_stride_frames, uint64_t* frames_out, const char** err);

/* vsyn_pcm_spectral_host on the PCM of the most recent submit resampled to out_rate (what vsyn_resample_device followed by
 * vsyn_spectral_device at out_rate gives), without the PCM leaving the device. in_rates[S] as for vsyn_pcm_resample_host;
 * the spec's fmin / fmax are checked against out_rate. Synchronous. */
int vsyn_pcm_resample_spectral_host(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t num_segments, const uint32_t* in_rates,
                                    uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status,
                                    const char** err);

/* ---- spectral post-processing: delta columns and mean / variance normalisation of spectral rows, computed where the rows are ----
 *
 * Input: one segment's spectral matrix X[f][d], F rows, D = dim columns (any of the four kinds). Output: a float32 matrix
 * (F, D_out), D_out = D * (1 + order). These are the options with_delta / norm_mean / norm_std_dev of RETURNN's
 * ExtractAudioFeatures; the deltas are librosa.feature.delta's. Neither is among the test dependencies: the device is compared
 * against a float64 model of the arithmetic below (tests/spectral_post_model.py), and the model's deltas against
 * scipy.signal.savgol_filter.
 *
 *  1. Deltas. width odd in [3, 65], h = (width - 1) / 2, k = -h .. h, S2 = sum k^2, S4 = sum k^4.
 *       c1[k] = k / S2;   c2[k] = 2 (width k^2 - S2) / (width S4 - S2^2).
 *     For h <= f <= F-1-h: D_o[f][d] = sum_k c_o[k] X[f+k][d], k ascending. For the h rows at either end:
 *     D_o[f] = D_o[clamp(f, h, F-1-h)]. This is scipy.signal.savgol_filter(X, width, deriv=o, polyorder=o, axis=0,
 *     mode="interp"), i.e. librosa.feature.delta(order=o): with polyorder equal to the derivative order the edge polynomial's
 *     o-th derivative is a constant, so the edge rows repeat the first / last interior row. Order 2 is the second derivative of
 *     X, not a delta of the delta. Y = [X | D_1 | D_2] up to `order`. A segment with 0 < F < width and order > 0 is an error (as
 *     in librosa); F = 0 gives (0, D_out).
 *  2. Normalisation, on Y, column by column, after the deltas (RETURNN's order).
 *     VSYN_POST_STATS_SEGMENT: mu[j] = (1/F) sum_f Y[f][j], sigma[j] = sqrt((1/F) sum_f (Y[f][j] - mu[j])^2) (numpy's std).
 *     VSYN_POST_STATS_GIVEN: mu = mean, sigma = std, the caller's float32 vectors of D_out entries (HOST arrays, read during the
 *     call; their length is the caller's word).
 *     VSYN_POST_NORM_MEAN: Z = Y - mu. VSYN_POST_NORM_MEAN_VAR: Z = (Y - mu) / max(sigma, std_floor): a constant column becomes zeros.
 *  3. Precision. The coefficients are rounded from double to float32; a delta is one float32 FMA chain in the order written. mu
 *     and sigma are accumulated in float64 in a fixed order: the sums of blocks of 16 rows of the segment, rows ascending; then
 *     16 chains, chain i adding the sums of blocks i, i + 16, ... in ascending order; then the chains in ascending order (no
 *     floating-point atomics). The order is a function of the segment's rows alone, so the result depends on neither the launch
 *     geometry nor the segment's place in the batch, and the same rows always give the same bits. Z = float32((double(Y) - mu) * r),
 *     r = 1 / max(sigma, std_floor) in float64 (1 for NORM_MEAN): one rounding to float32.
 *  4. Checks (VSYN_ERR_INVALID before anything runs): order <= 2; width odd in [3, 65] (whatever the order); norm and stats
 *     among the enums; std_floor finite and > 0; with given statistics and norm != none, mean non-NULL and finite, and for
 *     MEAN_VAR std non-NULL and finite.
 *  5. Not finite; nothing is refused. An Inf or NaN X[f][d] makes Y[f][d] and D_o[r][d] of every row r whose (clamped) window reads
 *     row f Inf or NaN (a coefficient of 0 as well: 0 * Inf is NaN); the h edge rows at either end have the window of the first /
 *     last interior row and go with it. Every other value of Y has the bits it has without it. With VSYN_POST_STATS_SEGMENT the mean and the deviation of
 *     each column of Y that holds such a value are not finite, and every row of that column of that segment is Inf or NaN (column
 *     d, and D + d, 2 D + d up to `order`); the other columns and the other segments are not touched.
 *
 * order = 0 with VSYN_POST_NORM_NONE launches nothing: the rows are those of the spectral entry points, bit for bit. The post
 * entry points read rows (and through vsyn_pcm_spectral_post_host, PCM) only: they touch neither stream state, the overlap buffers
 * nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One handle's post entry points share its post workspace. */
enum {
  VSYN_POST_NORM_NONE = 0,
  VSYN_POST_NORM_MEAN = 1,     /* "mean" */
  VSYN_POST_NORM_MEAN_VAR = 2  /* "mean_var" */
};
enum {
  VSYN_POST_STATS_SEGMENT = 0, /* per segment (RETURNN's "per_seq") */
  VSYN_POST_STATS_GIVEN = 1    /* the caller's mean / std */
};
#define VSYN_POST_MAX_WIDTH 65u

typedef struct vsyn_spectral_post {
  uint32_t order;     /* 0, 1 or 2 delta orders */
  uint32_t width;     /* odd, in [3, 65]; librosa's default is 9 */
  uint32_t norm;      /* VSYN_POST_NORM_* */
  uint32_t stats;     /* VSYN_POST_STATS_* */
  double std_floor;   /* > 0 */
  const float* mean;  /* VSYN_POST_STATS_GIVEN: [D_out], host */
  const float* std;   /* VSYN_POST_STATS_GIVEN with MEAN_VAR: [D_out], host */
} vsyn_spectral_post;

/* D_out = dim * (1 + order) for spec's dim; 0 for an invalid spec or post. */
uint32_t vsyn_spectral_post_dim(const vsyn_spectral_spec* spec, const vsyn_spectral_post* post);

/* The post stage alone on rows the caller has on the device (what vsyn_spectral_device wrote): d_in holds the segments' rows back
 * to back, dim columns (1 <= dim <= 256); seg_rows[S] is a HOST array of each segment's row count, so a segment with
 * 0 < F < width (order > 0) is refused by name before anything is launched. Writes d_out, the same rows with dim * (1 + order)
 * columns; d_out may be d_in only when order = 0. Asynchronous on hip_stream. */
int vsyn_spectral_post_device(vsyn_handle* h, const vsyn_spectral_post* post, uint32_t dim, uint32_t num_segments,
                              const uint64_t* seg_rows, const float* d_in, float* d_out, void* hip_stream, const char** err);

/* vsyn_pcm_spectral_host (out_rate = 0: each segment at its own rate) or vsyn_pcm_resample_spectral_host (out_rate != 0) followed
 * by the post stage, without rows or PCM leaving the device in between: rows receives D_out columns per row. A segment with
 * 0 < F < width (order > 0) makes the call VSYN_ERR_INVALID, with seg_rows filled. Synchronous. */
int vsyn_pcm_spectral_post_host(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_spectral_post* post, uint32_t num_segments,
                                const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                                vsyn_status* status, const char** err);

/* ---- PCM conditioning: mono downmix, peak normalisation and pre-emphasis of the decoded PCM, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames. Output: ONE float32 plane z[t] of the same T. This is
 * what the consumers of the spectral rows do to the waveform in front of the STFT: librosa.load(mono=True), and the options
 * peak_normalization / preemphasis of RETURNN's ExtractAudioFeatures. Neither is among the test dependencies: the device is
 * compared against a float64 model of the arithmetic below (tests/condition_model.py), and the model's pre-emphasis against
 * scipy.signal.lfilter.
 *
 *  1. Downmix. y[t] = the float32 sum of x[c][t] over the channels in ascending order, times float32(1 / C) when C > 1. It is the
 *     expression of step 1 of the spectral features, one device function shared by both: a mono plane from this stage, given to
 *     vsyn_spectral_device with channels = 1, gives the rows the C-channel PCM gives, bit for bit.
 *  2. Peak (VSYN_COND_PEAK). p = max_t |y[t]| over the segment's T frames. y1[t] = y[t] / p, the correctly rounded float32
 *     division, when p > 0: the peak sample becomes exactly +-1. y1 = y when p = 0 (silence, T = 0). A peak that is not finite
 *     (an Inf or NaN sample) refuses that segment alone: its plane is zeros and its entry of the peaks array holds the value that
 *     is not finite; the other segments of the call are not affected. Without the option y1 = y and nothing is checked.
 *  3. Pre-emphasis (VSYN_COND_PREEMPH, coefficient a, 0 < a < 1, rounded once to float32). z[0] = y1[0], and
 *     z[t] = fmaf(-a, y1[t-1], y1[t]) for t > 0: scipy.signal.lfilter([1, -a], [1], y1) with zero initial state. Without the
 *     option z = y1.
 *  4. Order in the pipeline: decode, resample per channel (if asked), condition, then PCM out or STFT, then the post stage. The
 *     peak is the peak of what the STFT sees.
 *  5. Checks (VSYN_ERR_INVALID before anything runs): unknown option bits; VSYN_COND_PREEMPH with a coefficient that is not
 *     finite, or that as a double or rounded to float32 is outside (0, 1); channels = 0.
 *
 * Precision: p is a maximum, taken on the absolute values' bit patterns as unsigned integers (no floating-point atomics), so it
 * depends on neither the order nor the launch geometry nor the segment's place in the batch; every z[t] is a function of x[.][t-1],
 * x[.][t] and p alone. The same input always gives the same bits. A NULL vsyn_pcm_cond means the stage is off: nothing is launched
 * and every entry point that takes one returns what its counterpart without the stage returns, bit for bit; options = 0 is the
 * downmix alone. The conditioning entry points read PCM only: they touch neither stream state, the overlap buffers nor the PCM
 * kept by VSYN_SUBMIT_KEEP_PCM, and a later vsyn_pcm_fetch_host returns the same PCM. One handle's conditioning entry points share
 * its conditioning workspace. */
#define VSYN_COND_PEAK 1u     /* peak normalisation (step 2) */
#define VSYN_COND_PREEMPH 2u  /* pre-emphasis with the coefficient `preemphasis` (step 3) */

typedef struct vsyn_pcm_cond {
  uint32_t options;    /* VSYN_COND_* option bits; the downmix is implied by the stage */
  uint32_t reserved;
  double preemphasis;  /* a, with VSYN_COND_PREEMPH */
} vsyn_pcm_cond;

/* The caller's planar PCM: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) frames per segment (clamped to
 * plane_stride and to out_plane_stride). Writes d_out[g * out_plane_stride + t] for t < T(g), nothing past it. d_peaks[S] (device,
 * may be NULL): with VSYN_COND_PEAK each segment's p (step 2: a value that is not finite marks a refused segment), not written
 * without the option. d_out with d_frames is in the input form of vsyn_spectral_device with channels = 1. Asynchronous on
 * hip_stream. */
int vsyn_pcm_condition_device(vsyn_handle* h, const vsyn_pcm_cond* cond, uint32_t num_segments, const float* d_pcm, uint64_t plane_stride,
                              uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, float* d_peaks,
                              void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle (with or without VSYN_SUBMIT_KEEP_PCM), per segment resampled from
 * in_rates[S] (host; 0 skips the segment) to out_rate when out_rate != 0 (out_rate = 0: no resampling, in_rates is not read and
 * may be NULL), conditioned, and copied to the host. frames_out[S] (host) receives each segment's T. out (may be NULL when only
 * the counts are wanted) receives the mono planes, out[g * out_stride_frames + t]: VSYN_PCM_F32 float32, or VSYN_PCM_S16 int16
 * converted as vsyn_pcm_interleave_device does. Frames past a segment's T are zero. peaks_out[S] (host, may be NULL): each
 * segment's p with VSYN_COND_PEAK (not finite: the segment is refused, step 2), 0 without. An out_stride_frames below some
 * segment's T is VSYN_ERR_INVALID, with frames_out filled. Synchronous. */
int vsyn_pcm_condition_host(vsyn_handle* h, const vsyn_pcm_cond* cond, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                            int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, float* peaks_out, const char** err);

/* The whole front end on the PCM of the most recent submit without anything leaving the device in between: resample (out_rate != 0;
 * in_rates as for vsyn_pcm_spectral_post_host), condition (cond != NULL), spectral rows, post stage (post != NULL). With cond and
 * post NULL this is vsyn_pcm_spectral_host resp. vsyn_pcm_resample_spectral_host, with cond NULL vsyn_pcm_spectral_post_host.
 * peaks_out[S] (host, may be NULL) as for vsyn_pcm_condition_host: a refused segment's rows are those of its plane of zeros, to be
 * discarded by the caller. Synchronous. */
int vsyn_pcm_cond_spectral_host(vsyn_handle* h, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_post* post,
                                uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity,
                                uint64_t* seg_rows, float* peaks_out, vsyn_status* status, const char** err);

/* ---- PCM trimming: the silent head and tail of the decoded PCM cut off, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames. Parameters: frame_length L, 1 <= L <= 8192; hop_length H,
 * H >= 1; top_db, finite, 0 < top_db <= 200. Output: ONE mono float32 plane, out_frames, and (start, end). This is
 * librosa.effects.trim(y, top_db, ref=np.max, frame_length=L, hop_length=H) on the mono signal. librosa is not among the test
 * dependencies: the device is compared against a float64 model of the arithmetic below (tests/trim_model.py), and the model against
 * a restatement in librosa's own words (tests/test_trim_cpu.py).
 *
 *  1. Downmix. y[t] is step 1 of the conditioning stage, the one device function the STFT and the conditioning stage use. The
 *     decision and the output are taken on the mono signal: for a mono file that is librosa's decision. librosa's per-channel
 *     aggregate (aggregate=np.max over the channels' frame energies) for multichannel input is NOT built.
 *  2. Frame energies: librosa.feature.rms(center=True, pad_mode="constant"). For T >= 1, F = 1 + (T + 2 (L / 2) - L) / H frames
 *     (integer divisions), F = 0 when that numerator is negative or T = 0. ms[f] = (1 / L) sum_{i < L} y[f H - L / 2 + i]^2, with
 *     zeros outside [0, T). The squares and the sums are float64: a float32 squared is exact in float64, so only the summation
 *     rounds. The order of a frame's sum is a function of L alone: lane l of 64 adds the samples l, l + 64, ... in ascending
 *     order, the 64 partial sums are joined by a butterfly over the lane offsets 32, 16, 8, 4, 2, 1, and the sum is divided by L.
 *     It depends on neither the tile, the grid nor the segment's place in the batch.
 *  3. Decision: amplitude_to_db(rms, ref=np.max, amin=1e-5, top_db=None) > -top_db, written without logarithms.
 *     E[f] = max(ms[f], 1e-10); R = max(max_f ms[f], 1e-10); k = 10^(-top_db / 10), computed once on the host in double. Frame f
 *     is non-silent iff E[f] > R * k (one float64 product) or E[f] >= R. In real numbers the second clause adds nothing (k < 1)
 *     and this is librosa's predicate; in float64 it keeps a loudest frame non-silent for a top_db so small that R * k rounds
 *     to R. Parity with librosa at a rounding distance from the threshold is not claimed.
 *  4. Bounds. f0 and f1 are the first and the last non-silent frame: start = f0 * H, end = min(T, (f1 + 1) * H). With F = 0,
 *     start = end = 0. The frame that holds the maximum is always non-silent (k < 1), so a segment with F >= 1 is never trimmed
 *     to nothing. For all-zero PCM, or any signal below amin, every E[f] = R: nothing is cut and (start, end) = (0, T).
 *  5. Output: out[t] = y[start + t] for t < end - start; out_frames = end - start; nothing is written past it.
 *  6. Not finite. A segment with an Inf or NaN sample among its T frames (in any channel's contribution to y, whether or not a
 *     frame covers it) is refused alone: it gets (0, 0), out_frames 0, and its entry of the ref array (R) is not finite. The
 *     other segments of the call are not affected.
 *  7. Order in the pipeline: decode, resample per channel (if asked), downmix and trim, peak, pre-emphasis, then PCM out or STFT,
 *     then the post stage. The peak is the peak of the trimmed signal, the pre-emphasis starts at z[0] = y1[start], "fewer frames
 *     than the delta width" applies to the trimmed rows, and (start, end) are in samples of the resampled signal.
 *  8. Checks (VSYN_ERR_INVALID before anything runs): L or H out of range; top_db not finite or outside (0, 200]; channels = 0.
 *
 * Not built: the per-channel aggregate, a ref other than the maximum (librosa.effects.split: "PCM splitting" below). No floating-point atomics and no
 * atomics at all: the same PCM gives the same bits, alone, in any slot of a batch and at any alignment. A NULL vsyn_pcm_trim means
 * the stage is off: nothing is launched and every entry point that takes one returns what its counterpart without the stage
 * returns, bit for bit. The trim entry points read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept
 * by VSYN_SUBMIT_KEEP_PCM, and a later vsyn_pcm_fetch_host returns the same PCM. One handle's trim entry points share its trim
 * workspace. */
#define VSYN_TRIM_MAX_FRAME 8192u

typedef struct vsyn_pcm_trim {
  uint32_t frame_length; /* L */
  uint32_t hop_length;   /* H */
  double top_db;         /* in (0, 200] */
} vsyn_pcm_trim;

/* F of step 2 for a segment of `frames` PCM frames, 0 for an invalid spec. */
uint64_t vsyn_pcm_trim_num_frames(const vsyn_pcm_trim* trim, uint64_t frames);

/* The caller's planar PCM: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) frames per segment (clamped to
 * plane_stride and to out_plane_stride). Writes d_out[g * out_plane_stride + t] for t < out_frames(g), nothing past it;
 * d_out_frames[S] (device, uint32); d_bounds[S][2] (device, uint32: start, end); d_ref[S] (device, double, may be NULL): R, not
 * finite for a refused segment; d_ms (device, double, may be NULL): d_ms[g * ms_stride + f] = ms[f] for f < F(g), ms_stride at
 * least vsyn_pcm_trim_num_frames(trim, min(plane_stride, out_plane_stride)). d_out with d_out_frames is in the input form of
 * vsyn_pcm_condition_device and vsyn_spectral_device with channels = 1. Asynchronous on hip_stream. */
int vsyn_pcm_trim_device(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t num_segments, const float* d_pcm, uint64_t plane_stride,
                         uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, uint32_t* d_out_frames,
                         uint32_t* d_bounds, double* d_ref, double* d_ms, uint64_t ms_stride, void* hip_stream, const char** err);

/* vsyn_pcm_condition_host with the trim in front of the conditioning: resample (out_rate != 0), downmix and trim, condition (cond
 * may be NULL with a trim: the trimmed downmix as it is; peaks_out then holds zeros), PCM out as one mono plane per segment.
 * frames_out[S] receives each segment's out_frames; bounds_out[S][2] (uint32, may be NULL) its (start, end); refs_out[S] (double,
 * may be NULL) its R (not finite: refused, step 6); peaks_out as for vsyn_pcm_condition_host. out_stride_frames is checked against
 * the UNTRIMMED T, which is known before the launch and bounds the result; with out = NULL nothing is launched and frames_out
 * receives that untrimmed T. trim = NULL is vsyn_pcm_condition_host (bounds_out and refs_out are not written). Synchronous. */
int vsyn_pcm_trim_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, uint32_t num_segments, const uint32_t* in_rates,
                       uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out,
                       float* peaks_out, double* refs_out, const char** err);

/* vsyn_pcm_cond_spectral_host with the trim in it: resample, downmix and trim, condition (cond != NULL), spectral rows, post stage
 * (post != NULL). The row counts of the later stages are the host's to give, so this form reads the bounds back once between the
 * trim and the spectral launches (S * 8 bytes and one wait). seg_rows are the rows of the trimmed segments; a refused segment
 * (refs_out not finite) and, with post->order > 0, a segment trimmed to 0 < F < post->width get 0 rows and fail alone: the caller
 * sees the latter from bounds_out. With rows = NULL the resampler and the trim still run, for the counts. trim = NULL is
 * vsyn_pcm_cond_spectral_host (bounds_out and refs_out are not written). Synchronous. */
int vsyn_pcm_trim_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                const vsyn_spectral_post* post, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                                float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* bounds_out, float* peaks_out,
                                double* refs_out, vsyn_status* status, const char** err);

/* ---- PCM splitting: the non-silent intervals of the decoded PCM, and the signal with its silent stretches removed ----
 *
 * Input and parameters as for "PCM trimming": one segment's planar float32 PCM x[c][t], C channels, T frames; frame_length L,
 * hop_length H and top_db in a vsyn_pcm_trim, with the same checks. Output: n intervals (start_k, end_k), uint32 pairs in ascending
 * order; optionally ONE mono float32 plane, the joined signal, and out_frames. This is librosa.effects.split(y, top_db, ref=np.max,
 * frame_length=L, hop_length=H) on the mono signal. The device is compared against tests/split_model.py, and that model against a
 * restatement in librosa's own words (tests/test_split_cpu.py).
 *
 *  1. Downmix, frame energies, decision: steps 1 to 3 of "PCM trimming", by the same kernel and the same device functions: the
 *     same y, the same ms[f] in the same summation order, the same predicate E[f] > R * k || E[f] >= R with the same k.
 *  2. Intervals. A maximal run of non-silent frames [a, b) is the interval (a * H, min(b * H, T)). n <= (F + 1) / 2. Only the last
 *     interval can be clipped by T; when the last frame alone is non-silent and (F - 1) * H = T it is (T, T), listed as librosa lists
 *     it, and contributes no samples. The first start and the last end are (start, end) of "PCM trimming".
 *  3. Joined signal: out = y[start_0 : end_0] ++ y[start_1 : end_1] ++ ..., out_frames = sum_k (end_k - start_k); nothing is written
 *     past it. Equivalently: the hops y[f * H : min((f + 1) * H, T)] of the non-silent frames f in order, which is how it is gathered.
 *  4. F = 0: no intervals, out_frames = 0. All-zero PCM, or PCM below amin: one interval (0, T).
 *  5. Not finite (step 6 of "PCM trimming"): the segment is refused alone: n = 0, out_frames = 0, and its R is not finite.
 *  6. Order in the pipeline: decode, resample per channel (if asked), downmix and split, peak, pre-emphasis, then PCM out or STFT,
 *     then the post stage: the peak, the pre-emphasis, the frames and "fewer frames than the delta width" are those of the joined
 *     signal, and the intervals are in samples of the resampled signal. A call either trims or splits.
 *  7. Checks (VSYN_ERR_INVALID before anything runs): those of "PCM trimming", and an intervals_stride below
 *     vsyn_pcm_split_max_intervals for the longest segment the call can hold.
 *
 * Integer scans and reductions only behind the energies, no atomics: the same PCM gives the same intervals and the same bits, alone,
 * in any slot of a batch and at any alignment. Entries of an interval array past a segment's count are not written by the device
 * entry and unspecified in the host entries. A NULL vsyn_pcm_trim means the stage is off, as for the trim entry points. The split
 * entry points read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One
 * handle's split entry points share its split workspace, which is not the trim stage's. */

/* (F + 1) / 2 for a segment of `frames` PCM frames: the most intervals it can have. 0 for an invalid spec. */
uint64_t vsyn_pcm_split_max_intervals(const vsyn_pcm_trim* trim, uint64_t frames);

/* The caller's planar PCM as for vsyn_pcm_trim_device. Writes d_out[g * out_plane_stride + t] for t < out_frames(g), nothing past
 * it; d_out_frames[S] (device, uint32); d_counts[S] (device, uint32): n; d_intervals (device, uint32):
 * d_intervals[(g * intervals_stride + k) * 2 + {0, 1}] = start_k, end_k for k < n(g), intervals_stride at least
 * vsyn_pcm_split_max_intervals(trim, min(plane_stride, out_plane_stride)); d_ref and d_ms as for vsyn_pcm_trim_device. d_out with
 * d_out_frames is in the input form of vsyn_pcm_condition_device and vsyn_spectral_device with channels = 1. Asynchronous on
 * hip_stream. */
int vsyn_pcm_split_device(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t num_segments, const float* d_pcm, uint64_t plane_stride,
                          uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, uint32_t* d_out_frames,
                          uint32_t* d_counts, uint32_t* d_intervals, uint64_t intervals_stride, double* d_ref, double* d_ms,
                          uint64_t ms_stride, void* hip_stream, const char** err);

/* vsyn_pcm_trim_host with the split in the trim's place: resample (out_rate != 0), downmix and split, condition (cond may be NULL:
 * the joined downmix as it is), PCM out as one mono plane per segment. frames_out[S] receives each segment's out_frames;
 * counts_out[S] (uint32, may be NULL) its n; intervals_out (uint32, may be NULL) its intervals,
 * intervals_out[(g * intervals_stride + k) * 2 + {0, 1}], intervals_stride at least vsyn_pcm_split_max_intervals of the longest
 * unsplit T; refs_out and peaks_out as for vsyn_pcm_trim_host. out_stride_frames is checked against the UNSPLIT T; with out = NULL
 * nothing is launched and frames_out receives that unsplit T. trim = NULL is vsyn_pcm_condition_host (counts_out, intervals_out
 * and refs_out are not written). Synchronous. */
int vsyn_pcm_split_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, uint32_t num_segments, const uint32_t* in_rates,
                        uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* counts_out,
                        uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out, const char** err);

/* The intervals alone of the PCM of the most recent submit: resample (out_rate != 0), frame energies, intervals. The joined signal
 * is not made and no PCM is copied back. frames_out[S] receives each segment's (resampled, unsplit) T; counts_out, intervals_out
 * with intervals_stride, and refs_out as for vsyn_pcm_split_host. With counts_out = NULL nothing is launched: frames_out alone, from
 * which the caller sizes intervals_out. Synchronous. */
int vsyn_pcm_split_intervals_host(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t num_segments, const uint32_t* in_rates,
                                  uint32_t out_rate, uint64_t* frames_out, uint32_t* counts_out, uint32_t* intervals_out,
                                  uint64_t intervals_stride, double* refs_out, const char** err);

/* vsyn_pcm_trim_spectral_host with the split in the trim's place. This form reads out_frames back once between the split and the
 * spectral launches (with the counts, the intervals and the refs; one wait). frames_out[S] (may be NULL) receives each segment's
 * out_frames; seg_rows are the rows of the joined segments; a refused segment and, with post->order > 0, a segment joined to
 * 0 < F < post->width get 0 rows and fail alone: the caller sees the latter from frames_out. With rows = NULL the resampler and the
 * split still run, for the counts. trim = NULL is vsyn_pcm_cond_spectral_host (frames_out, counts_out, intervals_out and refs_out
 * are not written). Synchronous. */
int vsyn_pcm_split_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                 const vsyn_spectral_post* post, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                                 float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* counts_out,
                                 uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                 vsyn_status* status, const char** err);

/* ---- PCEN: per-channel energy normalisation of spectral rows, computed where the rows are ----
 *
 * Input: one segment's rows X[f][j], F rows, D columns, float32, non-negative: the rows of VSYN_SPEC_MEL_POWER or VSYN_SPEC_LIN_POWER
 * (power 1 or 2). Output: a float32 matrix (F, D). This is librosa.pcen(S.T * scale, sr=sr, hop_length=hop, gain, bias, power,
 * time_constant, eps, b, max_size=1).T (librosa >= 0.10): an adaptive gain control along time in place of a fixed log compression.
 * librosa is not among the test dependencies and parity with it is not claimed: the device is compared against a float64 model of the
 * arithmetic below (tests/pcen_model.py), and the model against a restatement in librosa's own words with scipy.signal.lfilter and
 * lfilter_zi (tests/test_pcen_cpu.py).
 *
 *  1. Scale. S = float32(X * float32(scale)): one rounding, exact for a power of two. librosa's documentation uses 2^31 for float
 *     PCM; the default of the Python layer is 1.
 *  2. Coefficient. b as given, or for b = 0: t = time_constant * sr / hop_length, b = (sqrt(1 + 4 t^2) - 1) / (2 t^2), in double on
 *     the host. sr is the rate the segment's rows were computed at (the resample target, else the segment's own), so b is per
 *     segment. q = 1 - b.
 *  3. Smoother. M[f] = b S[f] + q M[f-1], M[-1] = 1, per column, in float64. This is scipy.signal.lfilter([b], [1, b - 1], S,
 *     zi=lfilter_zi([b], [1, b - 1])), whose zi is 1 - b and is not scaled by S[0], exactly as librosa does it.
 *  4. Gain and compression, in float64, in librosa's log-space form: G = exp(-gain * (log(eps) + log1p(M / eps))), then
 *       power = 0:              Y = log1p(S * G)
 *       power != 0, bias = 0:   Y = exp(power * (log(S) + log(G)))     (S = 0 gives 0)
 *       otherwise:              Y = bias^power * expm1(power * log1p(S * G / bias))
 *     and one rounding to float32.
 *  5. Order in the pipeline: ..., STFT and filterbank, PCEN, delta / normalisation.
 *  6. Checks (VSYN_ERR_INVALID before anything runs): gain, bias, power finite and >= 0; eps, time_constant, scale finite and > 0;
 *     b = 0 (derive it) or in (0, 1]; with b = 0, hop_length >= 1 and a non-NULL rate array; dim >= 1. Through the spectral entry
 *     points a kind other than VSYN_SPEC_MEL_POWER or VSYN_SPEC_LIN_POWER is refused by name: its rows can be negative. librosa's
 *     max_size > 1, ref, zi and return_zf are not built.
 *  7. The device entry does not look at signs: a NaN or a negative input propagates as IEEE arithmetic and the model say, and a NaN
 *     poisons the rest of its column, as in librosa: Y is NaN from its row on, rows before it and the other columns keep their
 *     bits. A -Inf does the same (M = -Inf, log1p of it is NaN). A +Inf does not: its own row is NaN (S G = Inf * 0), but M stays
 *     +Inf behind it, so with gain > 0 the gain G is 0 and every later row of the column is the value of step 4 at G = 0, a finite
 *     0, again as in librosa; with gain = 0, G = exp(-0 * Inf) is NaN and the column is NaN from the row on.
 *
 * Precision and order. The smoother is a blocked scan whose decomposition is a function of the segment's rows alone: blocks of 64
 * rows counted from the segment's first row. Per (block, column) the block's zero-state response at its last row (the recurrence
 * from 0, rows ascending); per column over the blocks in ascending order carry[0] = 1, carry[k+1] = part[k] + q^64 carry[k] (q^64
 * in double from the host); then every block from its carry, rows ascending. All in float64, no atomics, and every term is
 * non-negative, so nothing cancels. The result depends on neither the launch geometry nor the segment's place in the batch: the
 * same rows give the same bits. The PCEN entry points read rows (and through the host forms, PCM) only: they touch neither stream
 * state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One handle's PCEN entry points share its PCEN workspace. */
typedef struct vsyn_spectral_pcen { /* 56 bytes */
  double gain;          /* >= 0; librosa's default is 0.98 */
  double bias;          /* >= 0; 2 */
  double power;         /* >= 0; 0.5 */
  double time_constant; /* > 0, seconds; 0.4. Read only when b = 0 */
  double eps;           /* > 0; 1e-6 */
  double b;             /* 0: derived from time_constant, the rate and the hop; else in (0, 1] */
  double scale;         /* > 0; the rows are multiplied by float32(scale) first */
} vsyn_spectral_pcen;

/* The coefficient b of step 2 for rows computed at sample_rate every hop_length samples (pcen->b itself when it is not 0). 0 for an
 * invalid spec, and for b = 0 with sample_rate = 0 or hop_length = 0. */
double vsyn_spectral_pcen_b(const vsyn_spectral_pcen* pcen, uint32_t sample_rate, uint32_t hop_length);

/* The stage alone on rows the caller has on the device (what vsyn_spectral_device wrote): d_in holds the segments' rows back to
 * back, dim columns; seg_rows[S] is a HOST array of each segment's row count; sample_rates[S] (HOST; may be NULL when b != 0) the
 * rate each segment's rows were computed at, 0 skips the segment (its rows are neither read nor written). Writes d_out, the same
 * rows, and nothing past them; d_out may be d_in. Asynchronous on hip_stream. */
int vsyn_spectral_pcen_device(vsyn_handle* h, const vsyn_spectral_pcen* pcen, uint32_t dim, uint32_t num_segments, const uint64_t* seg_rows,
                              const uint32_t* sample_rates, uint32_t hop_length, const float* d_in, float* d_out, void* hip_stream,
                              const char** err);

/* vsyn_pcm_trim_spectral_host and vsyn_pcm_split_spectral_host with the PCEN stage between the spectral rows and the post stage, in
 * place on the rows, without rows or PCM leaving the device: b is derived (b = 0) from the rate the spectral stage sees and
 * spec->hop_length. pcen = NULL is the entry without the stage, bit for bit; trim = NULL, cond = NULL and post = NULL mean what they
 * mean there. A spec->kind other than VSYN_SPEC_MEL_POWER or VSYN_SPEC_LIN_POWER with pcen != NULL is VSYN_ERR_INVALID. Synchronous. */
int vsyn_pcm_trim_spectral_pcen_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                     const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t num_segments,
                                     const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                                     uint32_t* bounds_out, float* peaks_out, double* refs_out, vsyn_status* status, const char** err);
int vsyn_pcm_split_spectral_pcen_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                      const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t num_segments,
                                      const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                                      uint64_t* frames_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride,
                                      float* peaks_out, double* refs_out, vsyn_status* status, const char** err);

/* ---- pitch: the fundamental frequency of the decoded PCM per frame (YIN), computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, and its sample rate sr. Parameters: frame_length L,
 * hop_length H, fmin, fmax, trough_threshold, VSYN_PITCH_CENTER. Output: a float32 matrix (F, 2), one row per frame: f0 in Hz, and
 * the cumulative-mean-normalised difference at the chosen lag (the aperiodicity that librosa.yin discards and that a caller
 * thresholds for voicing). This is librosa.yin(y, fmin, fmax, sr, frame_length=L, win_length=L / 2, hop_length=H,
 * trough_threshold, center, pad_mode="constant") (librosa >= 0.10) on the mono signal. librosa is not among the test dependencies
 * and parity with it is not claimed: the device is compared against a float64 model of the arithmetic below (tests/pitch_model.py),
 * and the model against a restatement in librosa's own words (tests/test_pitch_cpu.py).
 *
 *  1. Mono. y[t] is step 1 of the conditioning stage, the one device function every stage uses.
 *  2. Framing. W = L / 2 (integer division). VSYN_PITCH_CENTER pads L / 2 zeros on both sides. The frame count F is that of
 *     "spectral features" step 2 with n_fft = L and the same hop (vsyn_pitch_num_frames), so that row f lines up with row f of the
 *     spectral rows. z[i] = y_pad[f H + i] for i < L.
 *  3. Periods, per segment rate: p_min = max(floor(sr / fmax), 1), p_max = min(ceil(sr / fmin), L - W - 1), computed in double on the
 *     host per call. n = p_max - p_min + 1 lags.
 *  4. Difference function: d[tau] = sum_{j = 1 .. W} (z[j] - z[j + tau])^2 for tau = 1 .. p_max: librosa's sum, including its start
 *     at j = 1, in direct form and not through an FFT. Each difference is formed in float64 (exact for float32 samples) and each
 *     sum is ONE float64 fma chain with j ascending. librosa zeroes autocorrelation values below 1e-6 in magnitude; that guards the
 *     cancellation of its FFT route, which the direct form does not have, and is NOT reproduced: quiet frames keep their d.
 *  5. Cumulative mean normalisation: S[tau] = sum_{u = 1 .. tau} d[u] in float64; c[i] = d[p_min + i] / (S[p_min + i] / (p_min + i)
 *     + tiny) for i < n, tiny = 2.2250738585072014e-308. S comes from a scan in a fixed order, a function of p_max alone
 *     (csrc/vsyn_pitch.h states it); its terms are >= 0, so its relative error is at most (terms) * 2^-53.
 *  6. Troughs: trough[i] = c[i] < c[i-1] and c[i] <= c[i+1] for 0 < i < n - 1; trough[0] = c[0] < c[1]; trough[n-1] = c[n-1] <
 *     c[n-2]. i* is the first i with trough[i] and c[i] < trough_threshold; without one, the first index of the minimum of c.
 *     Integer "first index" reductions, no atomics.
 *  7. Parabolic shift, for 0 < i* < n - 1: a = (c[i*+1] + c[i*-1]) - 2 c[i*], b = (c[i*+1] - c[i*-1]) / 2, shift = -b / a if
 *     |b| < |a|, else 0; shift = 0 at either end.
 *  8. Row f: column 0 = float32(sr / (p_min + i* + shift)), computed in float64 and rounded once; column 1 = float32(c[i*]). An
 *     all-zero frame gives (sr / p_min, 0) exactly.
 *  9. Not finite. A segment with an Inf or NaN sample among its T frames (the trim stage's test, whether or not a frame covers the
 *     sample) is refused alone: every value of its F rows is NaN and its entry of the refused array is 1. The other segments of
 *     the call are not affected.
 * 10. Checks (VSYN_ERR_INVALID before anything runs): 4 <= L <= 8192; 1 <= H; unknown option bits; fmin, fmax and
 *     trough_threshold finite; 0 < fmin < fmax <= sr / 2 and n >= 2 for every segment's rate; 0 < trough_threshold <= 1. A rate
 *     of 0 skips the segment (0 rows).
 *
 * Not built: a win_length other than L / 2, composition with the trim, split and conditioning stages. The same PCM gives the
 * same bits, alone, in any slot of a batch and at any alignment. The pitch entry points read PCM only: they touch neither stream
 * state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM, and a later vsyn_pcm_fetch_host returns the same PCM. One
 * handle's pitch entry points share its pitch workspace, which is no other stage's. */
#define VSYN_PITCH_CENTER 1u /* pad frame_length/2 zeros on both sides (librosa's center=True) */

typedef struct vsyn_pitch_spec {
  uint32_t frame_length; /* L */
  uint32_t hop_length;   /* H */
  uint32_t options;      /* VSYN_PITCH_* bits */
  uint32_t reserved;     /* 0 */
  double fmin, fmax;     /* Hz */
  double trough_threshold;
} vsyn_pitch_spec;

/* F of step 2 for a segment of `frames` PCM frames, 0 for an invalid spec (the checks of step 10 that need no rate). */
uint64_t vsyn_pitch_num_frames(const vsyn_pitch_spec* spec, uint64_t frames);

/* The caller's planar PCM: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) PCM frames per segment (clamped to
 * plane_stride). sample_rates[S] is a HOST array; a rate of 0 skips the segment. Writes d_seg_row_off[S+1] (uint64, may be NULL):
 * segment g's rows are [d_seg_row_off[g], d_seg_row_off[g+1]) of d_rows, which must hold sum_g vsyn_pitch_num_frames(spec,
 * frames_g) rows of 2 columns (S * vsyn_pitch_num_frames(spec, plane_stride) always suffices); d_refused[S] (device, uint32, may
 * be NULL): 1 for a refused segment (step 9), else 0. Asynchronous on hip_stream. */
int vsyn_pitch_device(vsyn_handle* h, const vsyn_pitch_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                      const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows,
                      uint64_t* d_seg_row_off, uint32_t* d_refused, void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle, per segment of that submit, each segment resampled from in_rates[g]
 * to out_rate first when out_rate != 0 (0: at its own rate in_rates[g]; the periods are those of the rate the rows are computed
 * at). in_rates[S] (host); a rate of 0 skips the segment. seg_rows[S] receives each segment's row count; rows (may be NULL when only
 * the counts are wanted: nothing is launched) receives the rows of all segments back to back, 2 columns each, at most
 * rows_capacity rows (VSYN_ERR_INVALID with the counts filled if it is too small); refused_out[S] (uint32, may be NULL) as
 * d_refused. status as for vsyn_pcm_spectral_host. Synchronous. */
int vsyn_pcm_pitch_host(vsyn_handle* h, const vsyn_pitch_spec* spec, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                        float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status,
                        const char** err);

/* ---- pyin: voiced flags, voicing probabilities and a Viterbi-decoded fundamental frequency (pYIN), computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, and its sample rate sr. Parameters: frame_length L,
 * hop_length H, fmin, fmax, n_thresholds N, the caller's table beta_probs[N], boltzmann_parameter lam, resolution,
 * max_transition_rate, switch_prob s, no_trough_prob, VSYN_PYIN_CENTER. Output: a float32 matrix (F, 3), one row per frame: f0 in
 * Hz (the decoded pitch bin's frequency, written for unvoiced frames too), voiced (1.0 or 0.0) and voiced_prob. This is
 * librosa.pyin(y, fmin, fmax, sr, frame_length=L, win_length=L / 2, hop_length=H, n_thresholds, beta_parameters,
 * boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob, center, pad_mode="constant") (librosa >= 0.10)
 * on the mono signal, before fill_na, which the caller applies. librosa is not among the test dependencies and parity with it is
 * not claimed: the device is compared against a float64 model of the arithmetic below (tests/pyin_model.py), and the model against
 * a restatement in librosa's own words (tests/test_pyin_cpu.py). tiny = 2.2250738585072014e-308 throughout.
 *
 *  1. Shared steps. Mono, framing, the periods p_min .. p_max, the difference function d and c[i], i < n, are steps 1 to 5 of
 *     "pitch", bit for bit: one device function, called by both kernels.
 *  2. Troughs: trough[i] of "pitch" step 6, its end rules included. The troughs in ascending lag are i_0 < i_1 < .. < i_(K-1), with
 *     heights h_k = c[i_k]. A frame without a trough has no voiced observation.
 *  3. Thresholds: t_m = m * (1.0 / N) for 1 <= m < N and t_N = 1 (numpy.linspace(0, 1, N + 1)[1:] bit for bit; m / N is not).
 *     beta_probs[m], m = 1 .. N, are the differences of the Beta(a, b) distribution function at 0, t_1, .. t_N: the caller's table
 *     of N doubles (threshold_probs); this library has no incomplete-beta routine.
 *  4. Trough probabilities. below(k, m) = h_k < t_m; n_m = #{k : below(k, m)}; pos(k, m) = #{k' <= k : below(k', m)} - 1;
 *     prior(k, m) = ((1 - e^-lam) / (1 - e^(-lam n_m))) * e^(-lam pos(k, m)) (scipy.stats.boltzmann.pmf, in this order);
 *     P_k = sum_m below(k, m) * (prior(k, m) * beta_probs[m]): one float64 chain with m ascending. With g the first index of the
 *     minimum of h: P_g += no_trough_prob * (sum of beta_probs[m] over the m with not below(g, m), m ascending). No atomics: the
 *     same PCM gives the same bits. The work is O(K N).
 *  5. Candidates. Every trough with P_k > 0 gives period = p_min + i_k + shift(i_k) (shift: "pitch" step 7), f0 = sr / period,
 *     bin = clip(rint(12 bps log2(f0 / fmin)), 0, B), round half even, with bps = ceil(1 / resolution) and B = floor(12 bps
 *     log2(fmax / fmin)) + 1 computed in double on the host (vsyn_pyin_num_bins). A candidate at bin == B is dropped (librosa's
 *     clip to n_pitch_bins, whose slot its unvoiced fill overwrites). Of several candidates in one bin the one with the LARGEST lag
 *     gives the bin's value (numpy's last assignment). obs[f][b], b < B, is that value, else 0.
 *     vp[f] = clip(sum_b obs[f][b], 0, 1), b ascending in float64. Every unvoiced state observes (1 - vp[f]) / B.
 *  6. Transitions. msf = round(max_transition_rate * 12 * H / sr) (half even, Python's round) per segment rate; w = msf bps + 1.
 *     An EVEN w is refused (VSYN_ERR_INVALID): librosa's pad_center and roll make that case asymmetric and dependent on the parity
 *     of B; a stated divergence, which needs a resolution other than the default. With h = w / 2: loc[i][j] = ((w + 1) / 2 - |j - i|)
 *     / ((w + 1) / 2) for |j - i| <= h and 0 <= j < B, else 0 (scipy.signal.get_window("triangle", w, fftbins=False)); each row is
 *     divided by its sum, added from the outside in, the two entries of a distance first (sum += loc[i][i-d] + loc[i][i+d] for
 *     d = h .. 1, then loc[i][i]), so that the mirror rows i and B - 1 - i hold the same bits. The state of voicing v (0 voiced, 1 unvoiced) and bin i has index v B + i.
 *     trans = kron([[1 - s, s], [s, 1 - s]], loc), and the Viterbi uses log(trans + tiny): outside the band that is log(tiny), about
 *     -708.4, NOT -inf, and it is evaluated: a clean tone has vp == 1 exactly, so its unvoiced observations are log(tiny) too, and
 *     its back pointers do leave the band. The out-of-band term of a target is the maximum of value + log(tiny) over the states
 *     outside its band, taken from prefix and suffix maxima per frame, not from a dense (2B)^2 sweep. Interior rows (h <= i < B - h)
 *     are translates of one row; the log table is built on the host in double. vsyn_pyin_transition returns it without a device.
 *  7. Viterbi (librosa.sequence.viterbi). value[0][s] = log(obs[0][s] + tiny) + log(1 / (2B) + tiny);
 *     value[t][s'] = log(obs[t][s'] + tiny) + max_s (value[t-1][s] + log_trans[s][s']); the back pointer is the LOWEST s that
 *     attains the maximum (np.argmax); the last state is the lowest arg-max of the last frame's values; then the back pointers are
 *     walked. Every maximum is taken under the total order "greater value, then lower state", so no grouping changes it. One
 *     workgroup per segment, frames in sequence; value ping-pongs in LDS as float64. 2B <= VSYN_PYIN_MAX_STATES.
 *  8. Row f: column 0 = float32(fmin * 2^((state mod B) / (12 bps))) from a host table in double; column 1 = state < B;
 *     column 2 = float32(vp[f]).
 *  9. Not finite and skipped segments: as "pitch" step 9, a segment with an Inf or NaN sample is refused alone (its F rows NaN,
 *     its refused word 1; its observations are not decoded). A rate of 0 or T = 0 gives 0 rows.
 * 10. Checks (VSYN_ERR_INVALID before anything runs): those of "pitch" step 10 without the threshold; 1 <= N <= 1024; threshold_probs
 *     not NULL, every entry finite and >= 0; lam > 0 and finite; 0 < resolution < 1; max_transition_rate > 0 and finite;
 *     0 < switch_prob < 1; 0 <= no_trough_prob <= 1; 2B <= VSYN_PYIN_MAX_STATES; w odd for every segment's rate.
 *
 * Memory. Between the two kernels the observations are a dense float64 matrix (F, B) per segment in the stage's own workspace, and
 * the back pointers take 2 bytes per state and frame: 8 F B + 4 F B bytes a segment (and 8 F for vp), about 3 MB for 10 s at the
 * defaults (F = 431, B = 601). Not built: a sparse form of the observations; an even w; a win_length other than L / 2. The same PCM
 * gives the same bits, alone, in any slot of a batch and at any alignment. The entry points read PCM only, as the pitch stage's do,
 * and share the handle's pyin workspace, which is no other stage's. */
#define VSYN_PYIN_CENTER 1u /* pad frame_length/2 zeros on both sides (librosa's center=True) */
#define VSYN_PYIN_MAX_STATES 4096u

typedef struct vsyn_pyin_spec {
  uint32_t frame_length; /* L */
  uint32_t hop_length;   /* H */
  uint32_t options;      /* VSYN_PYIN_* bits */
  uint32_t n_thresholds; /* N */
  double fmin, fmax;     /* Hz */
  double boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob;
  const double* threshold_probs; /* beta_probs[N] of step 3 (host) */
} vsyn_pyin_spec;

/* F of step 1 for a segment of `frames` PCM frames, 0 for an invalid spec (the checks of step 10 that need no rate). */
uint64_t vsyn_pyin_num_frames(const vsyn_pyin_spec* spec, uint64_t frames);

/* B of step 5, 0 for an invalid spec. */
uint32_t vsyn_pyin_num_bins(const vsyn_pyin_spec* spec);

/* Host only, no device and no handle: w of step 6 at rate sample_rate into *width_out and B into *bins_out (either may be NULL), and,
 * when table is not NULL, the log table of step 6: table[(i * w + k) * 2 + x] for the source bin i < B, the target bin j = i + k - h,
 * k < w, and x = 0 for the same voicing (log((1 - s) loc[i][j] + tiny)), 1 for the other (log(s loc[i][j] + tiny)); log(tiny) where
 * j is outside [0, B). table_capacity counts doubles: VSYN_ERR_INVALID (with w and B filled) below B * w * 2. */
int vsyn_pyin_transition(const vsyn_pyin_spec* spec, uint32_t sample_rate, uint32_t* width_out, uint32_t* bins_out, double* table,
                         uint64_t table_capacity, const char** err);

/* The caller's planar PCM, as for vsyn_pitch_device; d_rows holds rows of 3 columns. */
int vsyn_pyin_device(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                     const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows,
                     uint64_t* d_seg_row_off, uint32_t* d_refused, void* hip_stream, const char** err);

/* The Viterbi of steps 6 and 7 alone, the second kernel of vsyn_pyin_device: d_obs (device, float64) holds the caller's dense
 * observation rows (seg_rows[g], B) of the segments back to back, every value finite and in [0, 1] (other values give states in
 * range that mean nothing); vp of a frame is step 5's clipped sum of its row. seg_rows[S] and sample_rates[S] are HOST arrays; a
 * rate of 0 skips the segment (its rows are still counted in the offsets). Writes d_states (device, uint32): the state of every
 * frame, back to back as the rows are. Asynchronous on hip_stream. */
int vsyn_pyin_decode_device(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                            const double* d_obs, const uint64_t* seg_rows, uint32_t* d_states, void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle, as for vsyn_pcm_pitch_host; rows of 3 columns. */
int vsyn_pcm_pyin_host(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                       float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status,
                       const char** err);

/* ---- frame descriptors: energy, zero-crossing rate and spectral shape of the decoded PCM per frame, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, and its sample rate sr. Parameters: n_fft, hop_length,
 * win_length, roll_percent, zcr_threshold, amin, VSYN_FDESC_CENTER. Output: a float32 matrix (F, 6), one row per frame, the columns
 * in this order: rms, zcr, centroid, bandwidth, rolloff, flatness, as librosa.feature.rms (pad_mode="constant"),
 * zero_crossing_rate (edge padding, threshold=zcr_threshold), spectral_centroid, spectral_bandwidth (p=2), spectral_rolloff and
 * spectral_flatness (power=2) define them on the mono signal. librosa is not among the test dependencies and parity with it is not
 * claimed: the device is compared against a float64 model of the arithmetic below (tests/fdesc_model.py), and the model against a
 * restatement with numpy.fft.rfft (tests/test_fdesc_cpu.py).
 *
 *  1. Mono and framing. y[t] is step 1 of the conditioning stage, the one device function every stage uses. The frame count F is
 *     that of "spectral features" step 2 with the same n_fft, hop and centring (vsyn_fdesc_num_frames), so that row f lines up with
 *     row f of the spectral rows and with frame f of the pitch stage at frame_length = n_fft. P = n_fft / 2 (integer division) with
 *     VSYN_FDESC_CENTER, else 0; frame f covers the samples t = f hop - P + j, j < n_fft.
 *  2. rms. y_j = y[t] inside [0, T) and 0 outside. E = sum_j y_j^2: every sample is widened to float64, the squares are added by
 *     fma in the order below (the samples dealt as the bins are, K = ceil(n_fft / 256)), and rms = sqrt(E / n_fft), rounded once to
 *     float32.
 *  3. zcr. Here a sample outside [0, T) is the nearest valid one (t clamped to [0, T - 1]). s_j = (y_j < 0 and |y_j| >
 *     zcr_threshold), compared in float64. zcr = #{1 <= j < n_fft: s_j != s_(j-1)} / n_fft, rounded once: the count is an integer
 *     and the column is exact.
 *  4. STFT. The window w is the spectral stage's: float32(0.5 - 0.5 cos(2 pi i / win_length)), i < win_length, placed at
 *     (n_fft - win_length) / 2 and 0 elsewhere; padding is zero as in step 2. v_j = (double)w_j * (double)y_j (exact). The twiddle
 *     table is float64, built on the host: (cos(a_m), sin(a_m)), a_m = 2.0 * pi * m / n_fft evaluated left to right in double,
 *     m < n_fft. For k = 0 .. n_fft / 2: re_k = sum_j v_j cos(a_(j k mod n_fft)), im_k likewise with sin, each ONE float64 fma chain
 *     with j ascending from 0.0; S_k = sqrt(fma(re_k, re_k, im_k im_k)). NB = n_fft / 2 + 1 bins.
 *  5. Ordered sums over k. With K = ceil(NB / 256), thread t of 256 owns the bins t K .. min((t + 1) K, NB) - 1 and adds its terms
 *     in ascending order from 0.0; the 256 totals are scanned in four groups of 64 (Hillis-Steele over the offsets 1, 2, .. 32),
 *     a group's offset is the sum of the earlier groups' totals in ascending order, and the sum over all bins is ((g0 + g1) + g2) +
 *     g3. c_k = (group offset + the exclusive prefix of the thread) + S_first + .. + S_k, left to right. A = c_(NB-1).
 *     f_k = (k * sr) / n_fft in double. A function of n_fft alone; every sum below is taken in this order, in float64.
 *  6. centroid = (sum_k fma(f_k, S_k, .)) / A. bandwidth = sqrt((sum_k fma(S_k d_k, d_k, .)) / A), d_k = f_k - centroid. If
 *     A < 1.1754944e-38 both are 0.
 *  7. rolloff. theta = roll_percent * A. k* is the first k with c_k >= theta (an integer minimum, no atomics); rolloff = f_(k*). A
 *     silent frame gives k* = 0.
 *  8. flatness. P_k = max(amin, S_k S_k). flatness = exp((sum_k ln P_k) / NB) / ((sum_k P_k) / NB).
 *  9. Not finite. A segment with an Inf or NaN sample among its T frames (the trim stage's test, whether or not a frame covers the
 *     sample) is refused alone: every value of its F rows is NaN and its entry of the refused array is 1. The other segments of
 *     the call are not affected.
 * 10. A rate of 0 skips the segment (0 rows); T = 0 gives 0 rows.
 * 11. Checks (VSYN_ERR_INVALID before anything runs): 16 <= n_fft <= 8192; 1 <= hop_length; 1 <= win_length <= n_fft;
 *     0 < roll_percent < 1; zcr_threshold finite and >= 0; amin finite and > 0; unknown option bits; channels >= 1; sample_rates
 *     non-NULL when there are segments.
 *
 * Every column is rounded to float32 once, from float64. Not built: composition with the trim, split and conditioning stages,
 * p != 2, selectable columns. The same PCM gives the same bits, alone, in any slot of a batch and at any alignment. The entry
 * points read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM, and a later
 * vsyn_pcm_fetch_host returns the same PCM. One handle's frame descriptor entry points share its frame descriptor workspace,
 * which is no other stage's. */
#define VSYN_FDESC_CENTER 1u /* pad n_fft/2 on both sides (librosa's center=True) */

typedef struct vsyn_fdesc_spec {
  uint32_t n_fft;
  uint32_t hop_length;
  uint32_t win_length;
  uint32_t options;     /* VSYN_FDESC_* bits */
  double roll_percent;  /* step 7 */
  double zcr_threshold; /* step 3 */
  double amin;          /* step 8 */
} vsyn_fdesc_spec;

/* F of step 1 for a segment of `frames` PCM frames, 0 for an invalid spec. */
uint64_t vsyn_fdesc_num_frames(const vsyn_fdesc_spec* spec, uint64_t frames);

/* The caller's planar PCM, as for vsyn_pitch_device: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) PCM frames
 * per segment (clamped to plane_stride), sample_rates[S] a HOST array (0 skips the segment). Writes d_seg_row_off[S+1] (uint64, may
 * be NULL) and d_rows, which must hold sum_g vsyn_fdesc_num_frames(spec, frames_g) rows of 6 columns; d_refused[S] (device, uint32,
 * may be NULL): 1 for a refused segment (step 9), else 0. Asynchronous on hip_stream. */
int vsyn_fdesc_device(vsyn_handle* h, const vsyn_fdesc_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                      const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows,
                      uint64_t* d_seg_row_off, uint32_t* d_refused, void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle, as for vsyn_pcm_pitch_host: each segment resampled from in_rates[g]
 * to out_rate first when out_rate != 0 (f_k then uses out_rate). seg_rows[S] receives each segment's row count; rows (may be NULL
 * when only the counts are wanted: nothing is launched) receives the rows of all segments back to back, 6 columns each, at most
 * rows_capacity rows (VSYN_ERR_INVALID with the counts filled if it is too small); refused_out[S] (uint32, may be NULL) as
 * d_refused. status as for vsyn_pcm_spectral_host. Synchronous. */
int vsyn_pcm_fdesc_host(vsyn_handle* h, const vsyn_fdesc_spec* spec, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                        float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status,
                        const char** err);

/* ---- constant-Q: the constant-Q / variable-Q transform of the decoded PCM and the chroma_cqt rows folded from it, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, and its sample rate sr. Parameters: n_bins,
 * bins_per_octave (bpo), hop_length, fmin, tuning, filter_scale, gamma, norm, VSYN_CQT_SCALE, an output selector and, for the chroma
 * outputs, n_chroma, chroma_norm and VSYN_CQT_BASE_C. This is the quantity librosa.cqt / librosa.vqt (window="hann",
 * pad_mode="constant") and librosa.feature.chroma_cqt approximate, in DIRECT TIME-DOMAIN FORM: every coefficient is the plain
 * sum of step 5 over the whole support of its wavelet. A stated divergence: librosa multiplies an STFT by a sparsified FFT basis
 * (its `sparsity`), octave by octave on a recursively decimated signal (its `res_type`, its early downsampling); none of the three
 * exists here, and none of their approximation errors. librosa is not among the test dependencies and parity with it is not
 * claimed: the device is compared against a float64 model of the arithmetic below (tests/cqt_model.py), and the model against closed
 * forms and a restatement as a correlation (tests/test_cqt_cpu.py).
 *
 *  1. Frequencies. f_k = (fmin * exp2(tuning / bpo)) * exp2(k / bpo), k < n_bins, in double in this order (the C library's exp2).
 *  2. Lengths. r = exp2(1 / bpo), alpha = (r r - 1) / (r r + 1), Q = filter_scale / alpha, N_k = (Q * sr) / (f_k + gamma / alpha), a
 *     double. gamma = 0 is the CQT, gamma > 0 the VQT; it costs nothing beyond the host table. N_k falls with k: bin 0 is the longest.
 *  3. Support and window. With h_k = ceil(N_k / 2), the support is the integers m in [-h_k, floor(N_k / 2)); their count L_k =
 *     h_k + floor(N_k / 2) is odd unless N_k / 2 is an integer, and h_k = ceil(L_k / 2). The window is the periodic Hann over the
 *     support: w_k[j] = 0.5 - 0.5 cos(2 pi j / L_k), j = m + h_k.
 *  4. Wavelet. b_k[m] = w_k[j] * exp(-2 pi i f_k m / sr) / n_k: re = w cos(p) / n_k, im = -(w sin(p)) / n_k with
 *     p = ((2 pi f_k) m) / sr; n_k = sum_j w_k[j] for norm 1 (the default), sqrt(sum_j w_k[j]^2) for norm 2, 1 for norm 0 (none),
 *     the sums added in ascending j. Built in double on the host, once per distinct rate, and stored as float32 pairs.
 *  5. Transform. y[t] is step 1 of the conditioning stage (the float32 downmix, the one device function every stage uses).
 *     C[t][k] = s_k * sum_m y[t hop + m] b_k[m], samples outside [0, T) taken as zero (librosa's pad_mode="constant", always
 *     centred); s_k = sqrt(N_k) with VSYN_CQT_SCALE (librosa's scale=True, the default), else N_k, stored as float32.
 *     F = 1 + T / hop (integer division; vsyn_cqt_num_frames) and T = 0 gives 0 rows. Row t is centred on sample t hop: where row t
 *     of every centred spectral kind with an even n_fft, and frame t of the centred pitch and descriptor stages, are centred.
 *     Order of one (t, k) sum, float32 throughout: the offsets m are cut into chunks [c K - K/2, (c + 1) K - K/2) of K =
 *     VSYN_CQT_CHUNK samples, the same grid for every bin, rate and batch; inside a chunk lane l of 64 runs one fma chain per
 *     component over the bin's offsets first + l, first + l + 64, .. (ascending; first = the larger of the chunk's and the support's
 *     first offset), the 64 chains go through the xor butterfly (offsets 32 .. 1), and the chunks' sums are added in ascending
 *     order onto 0.0. A fixed function of (L_k, K). No atomics.
 *  6. Outputs. VSYN_CQT_MAG: |C|^power, power 1 or 2 (sqrtf(fma(re, re, im im)) or the argument of the root), float32 (F, n_bins).
 *     VSYN_CQT_COMPLEX: re and im interleaved, (F, 2 n_bins), a complex64 matrix (F, n_bins) as the spectral kind "stft" is.
 *     VSYN_CQT_CHROMA: step 7, (F, n_chroma). VSYN_CQT_TONNETZ: step 8, (F, 6). vsyn_cqt_dim gives the columns.
 *  7. Chroma (librosa.feature.chroma_cqt with threshold=None, cqt_mode="full", window=None). R[c] = sum_k M[c][k] |C[t][k]|, the
 *     magnitudes (power is not read), added in ascending k in float32. M is librosa.filters.cq_to_chroma's 0/1 matrix: with
 *     n_merge = bpo / n_chroma (an integer), M[c][k] = 1 exactly for
 *       c = ((((k mod bpo) + n_merge / 2) mod bpo) / n_merge + roll) mod n_chroma        (integer divisions),
 *     roll = rint((n_chroma / 12.0) * m0) with VSYN_CQT_BASE_C and rint((n_chroma / 12.0) * (m0 - 9)) without, rint to even, reduced
 *     mod n_chroma to 0 .. n_chroma - 1, m0 = fmod(12 (log2(fmin) - log2(440)) + 69, 12) made non-negative (hz_to_midi of the
 *     UNTUNED fmin, as librosa has it). This is numpy's construction read out: repeat(eye(n_chroma), n_merge, axis=1) puts column j
 *     in class j / n_merge; roll(.., -(n_merge / 2), axis=1) makes column j the old column j + n_merge / 2; tile repeats the bpo
 *     columns; roll(.., roll, axis=0) moves class c to row c + roll. At fmin = C1 bin 0 is row 0 with VSYN_CQT_BASE_C and row 3
 *     (A = 0) without. Then the per-frame norm chroma_norm (VSYN_CHROMA_NORM_*), its FLT_MIN rule and the non-finite rule of
 *     "chroma" step 3: the same device function.
 *  8. Tonnetz. Step 4 of "chroma" applied to the rows of step 7: the same device function.
 *  9. Not finite. A segment with an Inf or NaN sample among its T frames is refused alone: every value of its F rows is NaN and its
 *     entry of the refused array is VSYN_CQT_NOT_FINITE (1): the descriptor stage's rule.
 * 10. Rate. A segment whose top bin's pass band leaves the Nyquist band, f_(n_bins-1) * (1 + 0.5 * 1.50018310546875 / Q) > sr / 2
 *     (the Hann window's bandwidth in bins, librosa's rule), is refused alone: its F rows are NaN and its entry of the refused array
 *     is VSYN_CQT_RATE (2); nothing of it is read, so this entry wins over step 9's. A rate of 0 skips the segment (0 rows).
 * 11. Checks (VSYN_ERR_INVALID before anything runs): 1 <= n_bins <= 256; 1 <= bpo <= 256; hop_length >= 1; fmin finite and > 0;
 *     filter_scale finite and > 0; gamma finite and >= 0; tuning finite; power 1 or 2; norm 0, 1 or 2; a known output; for the
 *     chroma outputs 1 <= n_chroma <= 256, bpo a multiple of n_chroma and a known chroma_norm; unknown option bits; channels >= 1;
 *     and for every rate of the call that step 10 does not refuse: L_0 <= VSYN_CQT_MAX_LENGTH (2^17) and sum_k L_k <=
 *     VSYN_CQT_MAX_TABLE (2^23 pairs, 64 MB).
 *
 * Deliberately not built: librosa's FFT-basis route and its sparsity; hybrid_cqt, pseudo_cqt, icqt, griffinlim_cqt; chroma_cens;
 * chroma_cqt's threshold and smoothing window; windows other than Hann; tuning = None inside vsyn_cqt_device (vsyn_pcm_cqt_est_host
 * below estimates first); dB output; composition with the trim, split, conditioning, delta, normalisation and HPSS stages; MFMA. The same PCM gives the same bits, alone, in any slot of a
 * batch and at any alignment. The entry points read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept
 * by VSYN_SUBMIT_KEEP_PCM. One handle's constant-Q entry points share its constant-Q workspace, which is no other stage's; the
 * wavelet tables of the last call's spec and (rate, tuning) pairs stay there, on the host and on the device. */
#define VSYN_CQT_SCALE 1u  /* s_k = sqrt(N_k) (librosa's scale=True) */
#define VSYN_CQT_BASE_C 2u /* chroma outputs: row 0 is C, else A */
#define VSYN_CQT_MAG 1u
#define VSYN_CQT_COMPLEX 2u
#define VSYN_CQT_CHROMA 3u
#define VSYN_CQT_TONNETZ 4u
#define VSYN_CQT_NOT_FINITE 1u /* refused[g], step 9 */
#define VSYN_CQT_RATE 2u       /* refused[g], step 10 */
#define VSYN_CQT_CHUNK 1024u
#define VSYN_CQT_MAX_LENGTH (1u << 17)
#define VSYN_CQT_MAX_TABLE (1u << 23)
#define VSYN_CQT_RATE_REFUSED 100 /* vsyn_cqt_lengths: the rate is refused under step 10 */

typedef struct vsyn_cqt_spec {
  uint32_t n_bins;
  uint32_t bins_per_octave;
  uint32_t hop_length;
  uint32_t options;     /* VSYN_CQT_SCALE, VSYN_CQT_BASE_C */
  uint32_t output;      /* VSYN_CQT_MAG .. VSYN_CQT_TONNETZ */
  uint32_t power;       /* 1 or 2 (VSYN_CQT_MAG) */
  uint32_t norm;        /* 0 (none), 1 or 2: step 4 */
  uint32_t n_chroma;    /* chroma outputs */
  uint32_t chroma_norm; /* VSYN_CHROMA_NORM_*, chroma outputs */
  uint32_t reserved;    /* 0 */
  double fmin, tuning, filter_scale, gamma;
} vsyn_cqt_spec;

/* Columns of a row (step 6), 0 for an invalid spec (the checks of step 11 that need no rate). */
uint32_t vsyn_cqt_dim(const vsyn_cqt_spec* spec);

/* F of step 5 for a segment of `frames` PCM frames, 0 for an invalid spec. */
uint64_t vsyn_cqt_num_frames(const vsyn_cqt_spec* spec, uint64_t frames);

/* Host only, no device and no handle: N_k and L_k of steps 2 and 3 at rate sample_rate into N[n_bins] and L[n_bins] (either may be
 * NULL). VSYN_ERR_INVALID for an invalid spec or a rate of 0 (nothing written); VSYN_CQT_RATE_REFUSED where step 10 refuses the
 * rate and VSYN_ERR_INVALID where L_0 or sum_k L_k exceed their caps, both with N and L filled; else VSYN_OK. */
int vsyn_cqt_lengths(uint32_t sample_rate, const vsyn_cqt_spec* spec, double* N, uint32_t* L);

/* Host only: the float32 pairs of bin k at rate sample_rate (step 4) into re_im[2 L_k], index 2 j and 2 j + 1, j = m + h_k: what
 * the device's table holds. The return values of vsyn_cqt_lengths; nothing is written unless VSYN_OK. */
int vsyn_cqt_basis(uint32_t sample_rate, const vsyn_cqt_spec* spec, uint32_t k, float* re_im);

/* Host only: M of step 7 into out[c * n_bins + k], n_chroma rows. VSYN_ERR_INVALID unless spec is valid with a chroma output. */
int vsyn_cq_to_chroma(const vsyn_cqt_spec* spec, float* out);

/* Host only, tuning facts for tests: out[0] frames per workgroup, out[1] samples per chunk (VSYN_CQT_CHUNK), out[2] bins per
 * workgroup (consecutive k, so of similar length: one wave per bin). Functions of the spec alone today; the rate is taken so that
 * they may depend on it. VSYN_ERR_INVALID for an invalid spec. */
int vsyn_cqt_tile(const vsyn_cqt_spec* spec, uint32_t sample_rate, uint32_t out[3]);

/* The caller's planar PCM, as for vsyn_fdesc_device: d_pcm[(g * channels + c) * plane_stride + t], d_frames[S] (device) PCM frames
 * per segment (clamped to plane_stride), sample_rates[S] a HOST array (0 skips the segment). Writes d_seg_row_off[S+1] (uint64, may
 * be NULL) and d_rows, which must hold sum_g vsyn_cqt_num_frames(spec, frames_g) rows of vsyn_cqt_dim(spec) columns; d_refused[S]
 * (device, uint32, may be NULL): 0, VSYN_CQT_NOT_FINITE or VSYN_CQT_RATE. Asynchronous on hip_stream. */
int vsyn_cqt_device(vsyn_handle* h, const vsyn_cqt_spec* spec, uint32_t num_segments, const uint32_t* sample_rates, const float* d_pcm,
                    uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off,
                    uint32_t* d_refused, void* hip_stream, const char** err);

/* The PCM of the MOST RECENT vsyn_submit_host* on this handle, as for vsyn_pcm_fdesc_host: each segment resampled from in_rates[g]
 * to out_rate first when out_rate != 0 (the wavelets are then those of out_rate). seg_rows[S] receives each segment's row count;
 * rows (may be NULL when only the counts are wanted: nothing is launched) receives the rows of all segments back to back, at most
 * rows_capacity rows (VSYN_ERR_INVALID with the counts filled if it is too small); refused_out[S] (uint32, may be NULL) as
 * d_refused. status as for vsyn_pcm_spectral_host. Synchronous. */
int vsyn_pcm_cqt_host(vsyn_handle* h, const vsyn_cqt_spec* spec, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                      float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status,
                      const char** err);

/* vsyn_pcm_cqt_host with each segment's tuning estimated first ("tuning estimation"; librosa's tuning = None). estimate NULL: that
 * entry, tuning_out not written. Otherwise estimate->bins_per_octave must equal spec->bins_per_octave; spec->tuning is still checked
 * and is not used. The estimate runs on the mono signal the transform sees (after the resampler) with librosa.cqt's own framing of
 * it: n_fft 2048, hop 512, Hann, centred, power 1. The tunings are read back (one more wait), the wavelets are built on the host by
 * the one builder for the distinct (rate, tuning) pairs of the call, and a segment's table entry indexes the pairs: segment g's rows
 * are, bit for bit, those of vsyn_pcm_cqt_host called with spec->tuning = tuning_out[g]. The handle keeps ONE wavelet table, the
 * last call's: a tuning is a multiple of 1 / nbin, so a call holds at most nbin = ceil(1 / resolution) sets of wavelets per rate,
 * each under the caps of step 11, and a call whose sets exceed the table's 4 GiB is refused by name. tuning_out[S] receives the
 * estimates (0.0 for a segment of rate 0). */
int vsyn_pcm_cqt_est_host(vsyn_handle* h, const vsyn_cqt_spec* spec, const vsyn_tuning_spec* estimate, uint32_t num_segments,
                          const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                          uint32_t* refused_out, double* tuning_out, vsyn_status* status, const char** err);

/* ---- loudness: the integrated loudness of the decoded PCM (ITU-R BS.1770-4 / EBU R 128) and the gain to a target, computed where the PCM is ----
 *
 * Input: one segment's planar float32 PCM x[c][t], C channels, T frames, at rate fs. The measured signal is the C planes
 * (VSYN_LOUD_SUM, Cs = C) or their mono downmix, the float32 expression of "PCM conditioning" step 1 (VSYN_LOUD_MONO, Cs = 1).
 * This is what pyloudnorm.Meter(fs).integrated_loudness and ffmpeg's ebur128 "I" compute for one and two channels; neither is among
 * the test dependencies and parity with them is not claimed: the device is compared against a float64 model of the arithmetic below
 * (tests/loudness_model.py), and the model against the standard's coefficient table, its 997 Hz calibration and EBU Tech 3341's
 * cases 1 to 5 (tests/test_loudness_cpu.py).
 *
 *  1. K-weighting. Two biquads in cascade, a high shelf and then a high pass, coefficients in double on the host from fs:
 *       shelf      G = 3.999843853973347 dB, Q = 0.7071752369554196, fc = 1681.974450955533,
 *                  K = tan(pi fc / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *                  b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],
 *                  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *       high pass  Q = 0.5003270373238773, fc = 38.13547087602444, b = [1, -2, 1], a by the same two expressions.
 *     At 48 kHz these are the standard's table to 8.9e-16. Each biquad runs in direct form II transposed in float64 from a zero
 *     state: scipy.signal.lfilter per section. vsyn_loudness_coefficients returns the ten numbers the device is given.
 *  2. Hops and blocks, in integers. Hop i covers the samples [(i fs) / 10, ((i + 1) fs) / 10) (integer division); Nh = (10 T) / fs
 *     whole hops. Block j is hops j .. j + 3, j < Nh - 3, and its mean square is z_j = (((s_j + s_j+1) + s_j+2) + s_j+3) / n_j with
 *     n_j its own sample count and s_i the float64 sum of the squared K-weighted samples of hop i, summed over the channels in
 *     ascending order with unit weights. With fs a multiple of 10 these are BS.1770-4's 400 ms blocks at 75 % overlap; at 11 025 and
 *     22 050 Hz the hop length alternates by one sample.
 *  3. Gating, on z with no logarithm on the device. Absolute gate: z_j > Z_abs = 10^((-70 + 0.691) / 10), a host double. zbar_a is
 *     the mean of the blocks kept. Relative gate: of those, z_j > zbar_a / 10.0. zbar is the mean of what is left; the integrated
 *     loudness is -0.691 + 10 log10(zbar), formed by the caller from zbar.
 *  4. Gain to a target L_t in LUFS (VSYN_LOUD_NORMALIZE): g = float32(sqrt(Z_t / zbar)), Z_t = 10^((L_t + 0.691) / 10) a host
 *     double; the division and the square root are the correctly rounded float64 ones, so float32(sqrt(Z_t / zbar)) formed from the
 *     record's zbar anywhere else is g bit for bit. y[t] = x[t] * g: one float32 multiplication, not clipped.
 *  5. The record per segment: zbar, zbar_a, the three block counts (all, above the absolute gate, above both), g (0 without a target
 *     or a measurement) and a status: VSYN_LOUD_OK; VSYN_LOUD_NOT_FINITE, a sample of the segment is Inf or NaN, the tail behind the
 *     last whole hop included; VSYN_LOUD_TOO_SHORT, Nh < 4; VSYN_LOUD_SILENT, no block passes the absolute gate;
 *     VSYN_LOUD_RATE_REFUSED, fs < 4000 (0 included): nothing of the segment is read. Where several hold the order is rate refused,
 *     not finite, too short, silent. A segment that is not VSYN_LOUD_OK has zbar = zbar_a = g = 0 and a scaled plane of zeros, as a
 *     refused segment has under VSYN_COND_PEAK.
 *  6. Checks (VSYN_ERR_INVALID before anything runs, outputs untouched): unknown option bits or channel mode, with
 *     VSYN_LOUD_NORMALIZE a target that is not finite or outside [-70, 0], NULL records, a scaled plane without VSYN_LOUD_NORMALIZE.
 *
 * Deliberately not built: BS.1770's surround weights (1.41) and its LFE exclusion, every channel has weight 1, so the result is the
 * standard's for one and two channels exactly; true peak, loudness range and short-term (3 s) or momentary loudness; any limiter.
 *  7. Order in the pipeline: resample, the gate (trim or split), loudness normalisation, conditioning (pre-emphasis), spectral rows,
 *     PCEN, delta / normalisation. As a step of a chain (vsyn_pcm_chain_host, vsyn_pcm_chain_spectral_host) the stage measures the
 *     mono plane the chain has at that point (the gated plane, else the downmix: VSYN_LOUD_MONO) at the rate the chain has there,
 *     and hands on y = x * g as 1-channel PCM. It excludes VSYN_COND_PEAK (VSYN_ERR_INVALID): two level controls. A segment that
 *     is not VSYN_LOUD_OK, a silent one included, hands on zeros and its record says why.
 *     Measured afresh the scaled signal need not be at L_t: the absolute gate does not move with the gain, so a block it cut can
 *     pass it afterwards. Over the blocks the measurement kept it is at L_t, up to float32.
 *
 * Precision and order. The filter is a blocked scan whose decomposition is a function of the segment's samples alone: chunks of 32
 * samples counted from the segment's first one, 256 chunks to a tile; the chunks' zero-state responses are combined with the powers
 * A^(32 2^k) of the cascade's 4x4 state-transition matrix, formed in double on the host, in a fixed order; tiles are chained in
 * ascending order. Sums of squares run per chunk in ascending order, per hop over its chunks in a fixed order, per gate over the
 * blocks in a fixed order. Float64 throughout, no atomics: the same PCM gives the same bits alone and anywhere in a batch. The
 * K-weighted samples differ from the float64 model's by rounding that leaves through the all-pole parts of the sections, whose
 * double pole near z = 1 amplifies it by about 1 / (1 - rho)^2; DESIGN.md 6m derives the bound the tests gate at. The entry points
 * read PCM only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One handle's
 * loudness entry points share its loudness workspace. */
#define VSYN_LOUD_NORMALIZE 1u /* form g for spec.target (step 4) */
enum {
  VSYN_LOUD_SUM = 0, /* the C planes, unit weights */
  VSYN_LOUD_MONO = 1 /* their mono downmix */
};
enum {
  VSYN_LOUD_OK = 0,
  VSYN_LOUD_NOT_FINITE = 1,
  VSYN_LOUD_TOO_SHORT = 2,
  VSYN_LOUD_SILENT = 3,
  VSYN_LOUD_RATE_REFUSED = 4
};
typedef struct vsyn_loudness_spec { /* 16 bytes */
  uint32_t options;      /* VSYN_LOUD_* bits */
  uint32_t channel_mode; /* VSYN_LOUD_SUM or VSYN_LOUD_MONO */
  double target;         /* L_t in LUFS, in [-70, 0]; read only with VSYN_LOUD_NORMALIZE */
} vsyn_loudness_spec;
typedef struct vsyn_loudness_record { /* 40 bytes */
  double zbar;         /* step 3; the integrated loudness is -0.691 + 10 log10(zbar) */
  double zbar_a;       /* the mean behind the absolute gate alone */
  uint32_t blocks;     /* Nh - 3, or 0 */
  uint32_t blocks_abs; /* of those, above the absolute gate */
  uint32_t blocks_rel; /* of those, above the relative gate too */
  float gain;          /* g of step 4 */
  uint32_t status;     /* VSYN_LOUD_OK ... */
  uint32_t reserved;
} vsyn_loudness_record;

/* The blocks of step 2 for a segment of `frames` frames at sample_rate: Nh - 3, 0 for Nh < 4 or a refused rate. */
uint64_t vsyn_loudness_num_blocks(uint32_t sample_rate, uint64_t frames);

/* The ten coefficients of step 1 at sample_rate as the device gets them: b0 b1 b2 a1 a2 of the shelf, then of the high pass.
 * VSYN_ERR_INVALID for a NULL out or a rate below 4000. */
int vsyn_loudness_coefficients(uint32_t sample_rate, double* out);

/* The nine 4x4 matrices A^(32 2^k), k = 0 .. 8, row-major, 144 doubles, of the cascade's state transition at sample_rate as the
 * device gets them ("Precision and order"). VSYN_ERR_INVALID for a NULL out or a rate below 4000. */
int vsyn_loudness_powers(uint32_t sample_rate, double* out);

/* The stage alone on the caller's planar PCM on the device: d_pcm[(g * channels + c) * plane_stride + t]; sample_rates[S] and
 * frames[S] are HOST arrays (frames clamped to plane_stride). Writes d_records[S]; d_z (may be NULL) receives the z_j of all
 * segments back to back, vsyn_loudness_num_blocks of them each (also for a segment that is not finite); d_weighted (may be NULL)
 * the K-weighted samples as float64, [(g * Cs + c) * weighted_plane_stride + t] (not written for a rate-refused segment);
 * d_scaled (may be NULL; needs VSYN_LOUD_NORMALIZE) the planes of step 4, [(g * Cs + c) * scaled_plane_stride + t], frames clamped
 * to the stride, nothing written past a segment's frames. Asynchronous on hip_stream. */
int vsyn_loudness_device(vsyn_handle* h, const vsyn_loudness_spec* spec, uint32_t num_segments, const uint32_t* sample_rates,
                         const uint64_t* frames, const float* d_pcm, uint64_t plane_stride, uint32_t channels,
                         vsyn_loudness_record* d_records, double* d_z, double* d_weighted, uint64_t weighted_plane_stride, float* d_scaled,
                         uint64_t scaled_plane_stride, void* hip_stream, const char** err);

/* The measurement of the PCM of the MOST RECENT vsyn_submit_host* on this handle, as for vsyn_pcm_pitch_host: each segment resampled
 * from in_rates[g] to out_rate first when out_rate != 0 (fs is then out_rate). records[S] receives the records (NULL: nothing is launched,
 * only seg_blocks is filled); seg_blocks[S] (may be NULL with records given) each segment's block count; z (may be NULL) the z_j of
 * all segments back to back, at most z_capacity of them (VSYN_ERR_INVALID with seg_blocks filled if it is too small). No PCM leaves the device. status as for vsyn_pcm_spectral_host.
 * Synchronous. */
int vsyn_pcm_loudness_host(vsyn_handle* h, const vsyn_loudness_spec* spec, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate,
                           vsyn_loudness_record* records, double* z, uint64_t z_capacity, uint64_t* seg_blocks, vsyn_status* status,
                           const char** err);

/* The most general PCM host form: vsyn_pcm_trim_host (gate_is_split = 0: bounds_out) or vsyn_pcm_split_host (gate_is_split != 0:
 * counts_out, intervals_out, intervals_stride) with the loudness step of "loudness" step 7 between the gate and conditioning. Every
 * stage's spec may be NULL (gate, loud, cond) and out_rate 0: that stage is off; loud = NULL is the entry without the argument, bit
 * for bit. With loud the output is one mono plane per segment, as with a gate or conditioning; loud needs VSYN_LOUD_NORMALIZE,
 * VSYN_LOUD_MONO and in_rates, and excludes VSYN_COND_PEAK (VSYN_ERR_INVALID, nothing written). records_out[S] (may be NULL)
 * receives the records. Behind a gate the call waits once more, for the gated frame counts. Synchronous. */
int vsyn_pcm_chain_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond,
                        uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, int format, void* out, uint64_t out_stride_frames,
                        uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride,
                        float* peaks_out, double* refs_out, vsyn_loudness_record* records_out, const char** err);

/* The most general spectral host form: vsyn_pcm_trim_spectral_pcen_host (gate_is_split = 0) or vsyn_pcm_split_spectral_pcen_host
 * (gate_is_split != 0) with the loudness step between the gate and conditioning; the rows are those of the normalised plane. NULL
 * specs, loud = NULL, the checks and records_out as for vsyn_pcm_chain_host; frames_out (may be NULL) the frames behind the gate. A
 * refused loudness spec leaves every output untouched, status included. Synchronous. */
int vsyn_pcm_chain_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                 const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_pcen* pcen,
                                 const vsyn_spectral_post* post, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                                 uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                                 uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                 vsyn_loudness_record* records_out, vsyn_status* status, const char** err);

/* vsyn_pcm_chain_spectral_host with the chroma parameters of "chroma" (NULL: the defaults) between spec and pcen. It runs through the
 * same chain body; with chroma = NULL and a kind other than CHROMA and TONNETZ it is that entry, bit for bit. */
int vsyn_pcm_chain_chroma_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                               const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                               const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t num_segments, const uint32_t* in_rates,
                               uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out,
                               uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out,
                               double* refs_out, vsyn_loudness_record* records_out, vsyn_status* status, const char** err);

/* vsyn_pcm_chain_chroma_host with each segment's tuning estimated first ("tuning estimation"; librosa's tuning = None). estimate NULL:
 * that entry, and tuning_out is not written. Otherwise spec->kind must be CHROMA or TONNETZ and estimate->bins_per_octave must equal
 * n_chroma (the unit of the tuning); chroma->tuning is still checked and is not used. The estimate runs on the PCM the chroma kernel
 * sees (after resample, trim or split, loudness and conditioning) at the call's own n_fft, hop_length, win_length, centring and
 * POWER: librosa's chroma_stft hands its power spectrogram to the estimator, and that quirk is kept. The tunings are read back (one
 * more wait; the entry is synchronous already), the filterbanks are built on the host by the one builder for the distinct
 * (rate, tuning) pairs of the call and kept for the next call with the same pairs, and the chroma kernels read a per-segment bank
 * index where they read the rate index otherwise: segment g's rows are, bit for bit, those of vsyn_pcm_chain_chroma_host called with
 * chroma->tuning = tuning_out[g]. tuning_out[S] receives the estimates (0.0 for a segment without rows). A call whose filterbanks
 * would exceed the table's 4 GiB is refused by name. */
int vsyn_pcm_chain_chroma_est_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                   const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                   const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_tuning_spec* estimate,
                                   uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity,
                                   uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                                   uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                   vsyn_loudness_record* records_out, double* tuning_out, vsyn_status* status, const char** err);

/* ---- HPSS: harmonic-percussive separation of spectral rows by median filtering, computed where the rows are ----
 *
 * Input: one segment's rows X[f][j], F rows (time), D columns (bins), float32: the rows of VSYN_SPEC_MEL_POWER or
 * VSYN_SPEC_LIN_POWER. Output: a float32 matrix (F, D). This is librosa.decompose.hpss(S.T, kernel_size=(kh, kp), power=power,
 * mask=..., margin=(margin_h, margin_p)) transposed, with scipy.ndimage.median_filter(mode="reflect") behind it. librosa is not among
 * the test dependencies and parity with it is not claimed: the contract is the arithmetic below, the device is compared against a
 * float64 model of it (tests/hpss_model.py), and the model against restatements in numpy's, scipy's and librosa's own words
 * (tests/test_hpss_cpu.py).
 *
 *  1. Medians. H[f][j] is the median of the kh values X[f - kh/2 .. f + kh/2][j] (along time), P[f][j] the median of the kp values
 *     X[f][j - kp/2 .. j + kp/2] (along bins); kh and kp are odd, k/2 is the integer quotient. An index outside the segment (or the
 *     row) is reflected as numpy.pad(mode="symmetric") does it, as often as needed: i mod 2n, and if that is >= n then 2n - 1 - that.
 *     F = 1 with kh = 63 is defined. Reflection is per segment: no value of a neighbouring segment is ever read. The median is a
 *     selection, not arithmetic: the element of rank k/2 of the window. H and P are therefore exact: equal as values to the model's
 *     (which of -0 and +0 comes back is not pinned). A window that holds a NaN gives NaN: sorting leaves that case undefined, so this
 *     is the rule here. -Inf and +Inf sort as numbers.
 *  2. Soft masks, in float64 (librosa.util.softmask). Harmonic: A = H, B = double(P) * margin_h. Percussive: A = P,
 *     B = double(H) * margin_p. Z = max(A, B) (a NaN operand gives NaN). Z < FLT_MIN: the element is "bad" and its mask is 0.5
 *     when both margins are 1, else 0. Otherwise, with a = (A / Z)^power and b = (B / Z)^power, the mask is a / (a + b).
 *     power = +Inf is the hard mask A > B (1 or 0). Non-finite values go through as IEEE arithmetic and the model say.
 *  3. Output, one of (each with one rounding to float32): the component X * mask; the mask; the median itself (H for the harmonic
 *     component, P for the percussive one), useful on its own as a noise-floor estimate.
 *  4. Order in the pipeline: ..., STFT and filterbank, HPSS, PCEN, delta / normalisation.
 *  5. Checks (VSYN_ERR_INVALID before anything runs, the output untouched): kh, kp odd and in [1, 63]; component and output known;
 *     margins finite and >= 1; power > 0, finite or +Inf; dim >= 1. Through the spectral entry points a kind other than
 *     VSYN_SPEC_MEL_POWER or VSYN_SPEC_LIN_POWER is refused by name, and so is PCEN together with the mask or the median output.
 *  6. Not built: even kernel sizes; the residual X - (harmonic + percussive); complex components as rows (the mask output applied
 *     to complex bins is the "inverse STFT" stage's mask argument, and "PCM effects" returns the component as PCM); both components
 *     from one call; HPSS in front of the chroma kinds, whose bins never leave the FFT workgroup.
 *
 * Precision and order. Step 1 selects out of LDS on order-preserving integer images of the floats, so denormals are neither flushed
 * nor reordered. Steps 2 and 3 are per element. Nothing is accumulated and no atomics are used: the result depends on neither the
 * launch geometry nor the segment's place in the batch, the same rows give the same bits. The HPSS entry points read rows (and
 * through the host form, PCM) only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM.
 * One handle's HPSS entry points share its HPSS workspace. */
enum { VSYN_HPSS_HARMONIC = 0, VSYN_HPSS_PERCUSSIVE = 1 };                            /* vsyn_spectral_hpss.component */
enum { VSYN_HPSS_OUT_COMPONENT = 0, VSYN_HPSS_OUT_MASK = 1, VSYN_HPSS_OUT_MEDIAN = 2 }; /* vsyn_spectral_hpss.output */

typedef struct vsyn_spectral_hpss { /* 40 bytes */
  uint32_t kh;        /* median length along time (harmonic), odd, 1 .. 63; librosa's default is 31 */
  uint32_t kp;        /* median length along bins (percussive), odd, 1 .. 63; 31 */
  uint32_t component; /* VSYN_HPSS_HARMONIC or VSYN_HPSS_PERCUSSIVE */
  uint32_t output;    /* VSYN_HPSS_OUT_* */
  double power;       /* > 0, finite or +Inf (hard mask); 2 */
  double margin_h;    /* finite, >= 1; 1 */
  double margin_p;    /* finite, >= 1; 1 */
} vsyn_spectral_hpss;

/* The stage alone on rows the caller has on the device (what vsyn_spectral_device wrote): d_in holds the segments' rows back to
 * back, dim columns; seg_rows[S] is a HOST array of each segment's row count. Writes d_out, the same rows, and nothing past them.
 * d_out may be d_in (the output then goes through the handle's HPSS workspace, grown on demand, and is copied back on the stream);
 * any other overlap of the two is not allowed. Asynchronous on hip_stream. */
int vsyn_spectral_hpss_device(vsyn_handle* h, const vsyn_spectral_hpss* hpss, uint32_t dim, uint32_t num_segments, const uint64_t* seg_rows,
                              const float* d_in, float* d_out, void* hip_stream, const char** err);

/* vsyn_pcm_chain_chroma_host with the HPSS stage between the spectral rows and PCEN, through the same chain body, without rows or
 * PCM leaving the device. hpss = NULL is that entry, bit for bit. With hpss != NULL a spec->kind other than VSYN_SPEC_MEL_POWER or
 * VSYN_SPEC_LIN_POWER, and pcen != NULL with an output other than VSYN_HPSS_OUT_COMPONENT, are VSYN_ERR_INVALID. Synchronous. */
int vsyn_pcm_chain_hpss_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                             const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                             const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                             uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity,
                             uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out,
                             uint64_t intervals_stride, float* peaks_out, double* refs_out, vsyn_loudness_record* records_out,
                             vsyn_status* status, const char** err);

/* ---- rhythm: onset strength, onset frames, tempogram, tempo and beats, computed where the rows are ----
 *
 * Three stages behind the spectral rows, and the beat tracker (D) behind the first of them: librosa.onset.onset_strength (aggregate = mean), librosa.onset.onset_detect through
 * util.peak_pick (backtrack = False), librosa.feature.tempogram (autocorrelation, window = "hann") and, on its mean,
 * librosa.feature.tempo (aggregate = mean, log-normal prior). librosa is not among the test dependencies and parity with it is not
 * claimed: the contract is the arithmetic below, the device is compared against a float64 model of it (tests/rhythm_model.py), and
 * the model against restatements in numpy's and scipy's own words (tests/test_rhythm_cpu.py).
 *
 * A. Onset strength. Input: one segment's rows S[f][j], F rows, D columns, 1 <= D <= 256, float32 (any kind; mel_db is what
 *    onset_strength(y, sr) feeds itself). Output: a float32 vector of exactly F entries.
 *  1. Reference rows. R = S when max_size = 1. Otherwise R[f][j] is the maximum of S[f][k], k in [j - m/2, j - m/2 + m), m = max_size,
 *     m/2 the integer quotient (scipy.ndimage.maximum_filter1d; even sizes are not centred). An index outside the row is reflected as
 *     numpy.pad(mode="symmetric") does it, as often as needed. A window that holds a NaN gives NaN.
 *  2. Envelope. p = n_fft / (2 hop_length) (integer quotient) with VSYN_ONSET_CENTER, else 0; g = f - p. env[f] = 0 when g < lag,
 *     else (1/D) sum_j max(0, double(S[g][j]) - double(R[g - lag][j])), where max(0, NaN) is NaN (numpy.maximum) and +-Inf go through
 *     as IEEE arithmetic says. F <= lag + p gives all zeros: the vector has F entries whatever librosa's center=False length would be.
 *  3. Order of the sum, a function of nothing at all: 64 partial sums, partial i adding its terms j = i, i + 64, i + 128, i + 192
 *     (those below D) in that order to 0.0, then six rounds o = 32, 16, 8, 4, 2, 1 in which partial i becomes partial i +
 *     partial (i xor o); partial 0 is the sum. It is divided by D in float64 and rounded once to float32.
 *  4. Checks (VSYN_ERR_INVALID before anything runs, outputs untouched): lag and max_size in [1, 64]; dim in [1, 256]; n_fft >= 1 and
 *     hop_length >= 1; no unknown option bit.
 *  5. Not built: aggregate = median, detrend, a caller's ref, onset_strength_multi's channels.
 *
 * B. Onset frames. Input: an envelope x of F float32 values per segment, that segment's sample rate. Output: the ascending list of
 *    onset frame indices, its count, and a refusal word.
 *  1. Window lengths in frames, per segment, on the host in double: w(t) = floor((t * rate) / hop_length); pre_max = w(pre_max
 *     seconds), post_max = w(post_max seconds) + 1, pre_avg = w(pre_avg seconds), post_avg = w(post_avg seconds) + 1, wait = w(wait
 *     seconds). librosa's defaults 0.03, 0.0, 0.10, 0.10, 0.03 give 1, 1, 4, 5, 1 at 22050 / 512. vsyn_onset_peak_windows returns them.
 *  2. Normalisation (VSYN_PEAKS_NORMALIZE): u[n] = (double(x[n]) - mn) / ((mx - mn) + FLT_MIN) in float64, mn and mx the segment's
 *     float32 minimum and maximum; otherwise u = double(x).
 *  3. Frame n is a candidate when (a) no x[k], k in [max(0, n - pre_max), min(F, n + post_max)), is greater than x[n] (on the float32
 *     values), and (b) u[n] >= sum / count + delta, the sum adding u[k], k in [max(0, n - pre_avg), min(F, n + post_avg)) in
 *     ascending order to 0.0 in float64, count the number of its terms.
 *  4. Walking n upwards, a candidate is accepted when none has been accepted yet or when n - last > wait (librosa >= 0.10.2's
 *     clipped-window loop). No special case for a constant envelope: the rule decides.
 *  5. A segment whose envelope holds an Inf or a NaN is refused: its word of the refusal array is 1 and its count 0.
 *  6. Checks: the five times finite and >= 0, delta finite, hop_length >= 1, every derived window <= 4096 frames, a rate of 0 skips
 *     the segment (count 0). At most ceil(F / (wait + 1)) frames are accepted.
 *
 * C. Tempogram. Input: an envelope e of F float32 values per segment. Output: float32 rows (F', W), time-major, and / or their
 *    mean over time g[W] in float64. W = win_length when that is not 0, else floor(ac_size * rate / hop_length) per segment (344 at
 *    22050 / 512 for librosa.feature.tempo's ac_size = 8 s), which vsyn_tempogram_win_length returns; W in [2, 2048].
 *  1. Padding. With VSYN_TG_CENTER e is padded by w = W/2 on both sides as numpy.pad(mode="linear_ramp", end_values=0) does it:
 *     left sample i is float(double(i) * (double(e[0]) / w)), right sample k counted from the edge outward float(double(w - 1 - k) *
 *     (double(e[F-1]) / w)). F' = F (0 when F = 0). Without it F' = max(0, F - W + 1).
 *  2. y_f[n] = double(win[n]) * double(e_pad[f + n]), exact in float64; win[n] = float(0.5 - 0.5 cos(2 pi n / W)) is built on the host
 *     in double (scipy.signal.get_window("hann", W, fftbins=True)). ac[f][l] = sum_{n = 0}^{W-1-l} y_f[n] y_f[n + l], one fma chain
 *     from 0.0 with n ascending, in float64.
 *  3. VSYN_TG_NORM_INF divides a row by mx = max_l |ac[f][l]| (a NaN among them makes mx NaN) unless mx <= FLT_MIN; without it the
 *     row is left as it is. Each output is rounded once to float32. Non-finite envelopes flow through as IEEE arithmetic says; with
 *     the norm a row whose window holds a NaN is NaN.
 *  4. Mean. g[l] = (sum over the F' rows of double(the float32 output)) / F'. With FT = vsyn_tempogram_tile(W) rows per tile, T =
 *     ceil(F' / FT) tiles, tpb = ceil(T / 128) tiles per block: a block's rows are added in ascending order to 0.0, then the blocks'
 *     sums in ascending order to 0.0; a function of W and F' alone. F' = 0 gives NaN.
 *  5. Tempo, on the host in double (vsyn_tempo_from_mean): bpm[0] = +Inf, bpm[l] = 60 rate / (hop_length l); logprior[l] = -0.5
 *     ((log2 bpm[l] - log2 start_bpm) / std_bpm)^2; with max_tempo > 0 the entries in front of the first lag whose bpm is below
 *     max_tempo are -Inf (no lag that slow: nothing is masked, numpy.argmax of an all-false array being 0: librosa's quirk, kept).
 *     The result is bpm[argmax_l(log1p(1e6 g[l]) + logprior[l])], the first index on a tie. A g that holds a non-finite value, or
 *     one below -1e-6 (log1p's domain), is refused with VSYN_ERR_INVALID.
 *  6. Checks: W in [2, 2048]; hop_length >= 1; ac_size finite and > 0 when win_length is 0; start_bpm and std_bpm finite and > 0;
 *     max_tempo finite and >= 0 (0: no cap).
 *  7. Not built: aggregate = None (a tempo per frame), a caller's prior, the Fourier tempogram, other windows and norms.
 *
 * D. Beat tracking: librosa >= 0.10.2's static-tempo beat tracker (librosa.beat.beat_track, units = "frames", sparse = True),
 *    restated. Input per segment: an envelope x of F float32 values and a period P in frames. Output: the ascending beat frames
 *    (uint32), their count and a refusal word. e = 2^-53; every sum is float64 in the stated order; no atomics on floating-point
 *    values. Model: tests/beat_model.py, with the bounds and the decision bands the device is gated on.
 *  0. Period, on the host in double (vsyn_beat_period): P = rint(60 (rate / hop_length) / bpm), half to even. bpm is the caller's, or
 *     the segment's tempo from C.5 with librosa.beat.beat_track's own defaults: ac_size 8 s, std_bpm 1, max_tempo 320 and the beat
 *     spec's start_bpm. P outside [1, 2048] refuses the segment with word 3; words 1 and 2 are a non-finite envelope and a tempo
 *     window length outside [2, 2048]. A segment with F < 2, or whose envelope has no non-zero value, is not refused: it has 0 beats
 *     and the chain reports bpm 0.0 (librosa's (0.0, [])).
 *  1. Normalise. m = (sum x) / F, sd = sqrt(sum (x - m)^2 / (F - 1)), u[n] = double(x[n]) / (sd + FLT_MIN). Order of both sums, a
 *     function of F alone: 256 partials, partial t adding its terms n = t, t + 256, .. in that order to 0.0 (a square is rounded
 *     before it is added); in each group of 64 consecutive partials six rounds o = 32, .., 1 in which partial i becomes partial i +
 *     partial (i xor o); then the four groups' sums in ascending order to 0.0.
 *  2. Local score. w[k] = exp(-0.5 (32 k / P)^2), k = -P .. P, built on the host in double. ls[i] = sum_k w[k] u[i - k] over the k
 *     with 0 <= i - k < F: one fma chain from 0.0 with k ascending. thr = 0.01 max_i ls[i]; i0 is the first i with ls[i] >= thr.
 *  3. Dynamic programme. h = rint(P / 2), half to even; lo = max(h, 1). tx[d] = -tightness (log d - log P)^2, d in [lo, 2P], a host
 *     table in double. For i ascending the candidates are loc = i - d, d = lo .. 2P, loc >= 0, with score s = cum[loc] + tx[d]; the
 *     best is the largest s, on a tie the smallest d. cum[i] = ls[i] + s_best, or ls[i] without a candidate. back[i] = loc_best
 *     (-1 without one) for i >= i0, and -1 for i < i0.
 *  4. Last beat. Frame i is a local maximum when cum[i] > cum[max(i - 1, 0)] and cum[i] >= cum[min(i + 1, F - 1)]. med is the
 *     median of cum over the local maxima (the mean of the two middle values for an even count). tail is the largest local maximum
 *     with cum >= 0.5 med, F - 1 if none qualifies. The beats are tail, back[tail], back[back[tail]], .. until -1, reversed. No local
 *     maximum: no beats.
 *  5. Trim (VSYN_BEAT_TRIM). With the beats b[0 .. B), v[j] = ls[b[j]], sm[j] = (0.5 v[j-1] + v[j]) + 0.5 v[j+1] with zeros outside,
 *     t = 0.5 sqrt((sum sm^2) / B), the sum ascending from 0.0, each square rounded first. Without the flag t = 0. The beats inside
 *     [n0, n1] are kept, n0 and n1 the first and the last frame with ls > t; no such frame: none.
 *  6. Checks (VSYN_ERR_INVALID before anything runs, outputs untouched): tightness and start_bpm finite and > 0; bpm finite and >= 0
 *     (0: estimated per segment; vsyn_beat_period wants one > 0); hop_length >= 1; no unknown option bit; segment sizes as everywhere
 *     in this section.
 *  7. Not built: the median aggregate of onset_strength that beat_track(y = ..) feeds itself (the envelope is A's mean aggregate),
 *     time-varying bpm, a caller's prior, units other than frames, sparse = False, plp.
 *
 * Order in the pipeline: ..., STFT and filterbank, HPSS, PCEN, onset strength, then peak picking, or tempogram and tempo, or
 * (tempogram mean, tempo and) beats.
 * Precision and order. No atomics; every accumulation order above is a function of the stage's parameters and the segment's row
 * count alone, so the same rows give the same bits anywhere in a batch and under any launch geometry. The entry points read rows
 * and envelopes only: they touch neither stream state, the overlap buffers nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One handle's
 * rhythm entry points share its rhythm workspace. */
enum { VSYN_ONSET_CENTER = 1u };                          /* vsyn_onset_spec.options */
enum { VSYN_PEAKS_NORMALIZE = 1u };                       /* vsyn_onset_peaks.options */
enum { VSYN_TG_CENTER = 1u, VSYN_TG_NORM_INF = 2u };      /* vsyn_tempogram_spec.options */

typedef struct vsyn_onset_spec { /* 20 bytes */
  uint32_t lag;        /* 1 .. 64; librosa's default is 1 */
  uint32_t max_size;   /* 1 .. 64; 1 */
  uint32_t n_fft;      /* of the rows' spectral spec: only p = n_fft / (2 hop_length) is used */
  uint32_t hop_length;
  uint32_t options;    /* VSYN_ONSET_CENTER */
} vsyn_onset_spec;

typedef struct vsyn_onset_peaks { /* 56 bytes */
  double pre_max, post_max, pre_avg, post_avg, wait; /* seconds; 0.03, 0.0, 0.10, 0.10, 0.03 */
  double delta;                                      /* 0.07 */
  uint32_t hop_length;
  uint32_t options; /* VSYN_PEAKS_NORMALIZE */
} vsyn_onset_peaks;

typedef struct vsyn_tempogram_spec { /* 24 bytes */
  uint32_t win_length; /* 2 .. 2048 (librosa.feature.tempogram's default is 384), or 0: from ac_size and each segment's rate */
  uint32_t hop_length;
  uint32_t options;    /* VSYN_TG_CENTER, VSYN_TG_NORM_INF */
  uint32_t reserved;   /* 0 */
  double ac_size;      /* seconds, read when win_length is 0; librosa.feature.tempo's default is 8.0 */
} vsyn_tempogram_spec;

typedef struct vsyn_tempo_spec { /* 24 bytes */
  double start_bpm; /* 120 */
  double std_bpm;   /* 1.0 */
  double max_tempo; /* 320; 0: no cap */
} vsyn_tempo_spec;

/* B.1: out[0 .. 4] = pre_max, post_max, pre_avg, post_avg, wait in frames for one rate. Pure host arithmetic; VSYN_ERR_INVALID as B.6. */
int vsyn_onset_peak_windows(const vsyn_onset_peaks* peaks, uint32_t sample_rate, uint32_t* out, const char** err);
/* C: W for one rate (0: the spec or the rate is refused), and the rows per tile of C.4 for a W (0: W outside [2, 2048]). */
uint32_t vsyn_tempogram_win_length(const vsyn_tempogram_spec* spec, uint32_t sample_rate);
uint32_t vsyn_tempogram_tile(uint32_t win_length);
/* C.5 for one segment's mean g[W]. Pure host arithmetic. lag_out may be NULL. */
int vsyn_tempo_from_mean(const vsyn_tempo_spec* tempo, const double* g, uint32_t win_length, uint32_t sample_rate, uint32_t hop_length,
                         double* bpm_out, uint32_t* lag_out, const char** err);

/* A on rows the caller has on the device: d_rows holds the segments' rows back to back, dim columns; seg_rows[S] is a HOST array of
 * each segment's row count. Writes d_env, one float per row, and nothing past them. Asynchronous on hip_stream. */
int vsyn_onset_strength_device(vsyn_handle* h, const vsyn_onset_spec* onset, uint32_t dim, uint32_t num_segments, const uint64_t* seg_rows,
                               const float* d_rows, float* d_env, void* hip_stream, const char** err);

/* B on envelopes the caller has on the device, back to back; seg_rows[S] and sample_rates[S] are HOST arrays. Segment g's accepted
 * frames go to d_onsets at the offset of its envelope (a segment never has more onsets than frames; the words behind its count are
 * left as they are), its count to d_counts[g], its refusal word to d_refused[g] (may be NULL). Asynchronous on hip_stream. */
int vsyn_onset_peaks_device(vsyn_handle* h, const vsyn_onset_peaks* peaks, uint32_t num_segments, const uint64_t* seg_rows,
                            const uint32_t* sample_rates, const float* d_env, uint32_t* d_onsets, uint32_t* d_counts, uint32_t* d_refused,
                            void* hip_stream, const char** err);

/* C on envelopes the caller has on the device, back to back; seg_rows[S] and sample_rates[S] (read only when win_length is 0; may be
 * NULL otherwise) are HOST arrays. d_rows (may be NULL): the segments' (F', W) matrices back to back. d_mean (may be NULL): the
 * segments' g[W] back to back, float64. Both NULL is refused. A W outside [2, 2048] for any segment is VSYN_ERR_INVALID; with
 * win_length 0 a rate of 0 skips its segment, which then has neither rows nor mean values.
 * Asynchronous on hip_stream. */
int vsyn_tempogram_device(vsyn_handle* h, const vsyn_tempogram_spec* spec, uint32_t num_segments, const uint64_t* seg_rows,
                          const uint32_t* sample_rates, const float* d_env, float* d_rows, double* d_mean, void* hip_stream,
                          const char** err);

/* What a host chain returns behind the onset stage (vsyn_rhythm_spec.output), as 32-bit words in its rows buffer; seg_rows[g] counts
 * the rows of segment g's output:
 *   ENVELOPE    F rows of 1 column: the envelope, float32;
 *   ONSETS      count rows of 1 column: the accepted frames, uint32 (peaks is read);
 *   TEMPOGRAM   F' rows of win_length columns, float32 (tempogram is read; its win_length must not be 0);
 *   TEMPO_MEAN  W + 1 rows of 2 columns, each row one float64: g[0 .. W-1], then the rate the rows were computed at (tempogram is
 *               read; W per segment). vsyn_tempo_from_mean turns g into the tempo. A segment without frames has no rows. */
enum { VSYN_RHYTHM_ENVELOPE = 0, VSYN_RHYTHM_ONSETS = 1, VSYN_RHYTHM_TEMPOGRAM = 2, VSYN_RHYTHM_TEMPO_MEAN = 3 };

typedef struct vsyn_rhythm_spec { /* 112 bytes */
  uint32_t output;   /* VSYN_RHYTHM_* */
  uint32_t reserved; /* 0 */
  vsyn_onset_spec onset; /* n_fft, hop_length and VSYN_ONSET_CENTER as the spectral spec has them */
  vsyn_onset_peaks peaks;
  vsyn_tempogram_spec tempogram;
} vsyn_rhythm_spec;

/* vsyn_pcm_chain_hpss_host with the rhythm stages behind pcen, through the same chain body, without rows, envelope or PCM leaving
 * the device: the onset stage takes the place of delta / normalisation, and a post spec that is on is refused together with it, by
 * name. rhythm = NULL is that entry, bit for bit (refused_out is then left alone). With rhythm != NULL: the kind's rows must have 1
 * to 256 columns; rows receives the selected output as words and rows_capacity counts WORDS, not rows (F words a segment suffice
 * for ENVELOPE and ONSETS, F win_length for TEMPOGRAM, 4098 for TEMPO_MEAN); seg_rows as above; refused_out[S] (may be NULL) is 1
 * for a segment whose envelope holds an Inf or a NaN (ONSETS: no frames) and 2 for one whose window length falls outside [2, 2048]
 * (TEMPO_MEAN: no rows); a rows of NULL only counts the spectral rows into seg_rows, as every chain entry does. Synchronous. */
int vsyn_pcm_chain_rhythm_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                               const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                               const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                               const vsyn_rhythm_spec* rhythm, uint32_t num_segments, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                               uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                               uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                               vsyn_loudness_record* records_out, uint32_t* refused_out, vsyn_status* status, const char** err);

enum { VSYN_BEAT_TRIM = 1u }; /* vsyn_beat_spec.options */

typedef struct vsyn_beat_spec { /* 32 bytes */
  double tightness;    /* 100 */
  double start_bpm;    /* 120: the prior of the tempo estimate */
  double bpm;          /* > 0: the caller's tempo for every segment; 0: estimated per segment (D.0) */
  uint32_t hop_length;
  uint32_t options;    /* VSYN_BEAT_TRIM */
} vsyn_beat_spec;

/* D.0 for one tempo and rate: *period_out = P, or 0 for a period outside [1, 2048]. Pure host arithmetic; VSYN_ERR_INVALID as D.6,
 * and for a bpm that is not finite and > 0, a rate of 0 or a NULL period_out. */
int vsyn_beat_period(const vsyn_beat_spec* beat, double bpm, uint32_t sample_rate, uint32_t* period_out, const char** err);

/* D.1 to D.5 on envelopes the caller has on the device, back to back; seg_rows[S] and periods[S] are HOST arrays. A period of 0
 * skips its segment: nothing of it is written. One above 2048 refuses it with word 3. Segment g's beats go to d_beats at the offset of
 * its envelope (never more beats than frames; the words behind its count are left as they are), its count to d_counts[g], its
 * refusal word (0, 1 or 3; count 0 with it) to d_refused[g] (may be NULL). d_localscore, d_cumscore (float64) and d_backlink (int32)
 * (each may be NULL) receive ls, cum and back at the envelope's offsets, for a segment that has a score (F >= 2, finite, not all
 * zero). The beat spec's bpm and start_bpm are checked and not read. Asynchronous on hip_stream. */
int vsyn_beat_track_device(vsyn_handle* h, const vsyn_beat_spec* beat, uint32_t num_segments, const uint64_t* seg_rows,
                           const uint32_t* periods, const float* d_env, uint32_t* d_beats, uint32_t* d_counts, uint32_t* d_refused,
                           double* d_localscore, double* d_cumscore, int32_t* d_backlink, void* hip_stream, const char** err);

/* vsyn_pcm_chain_rhythm_host's chain with the beat tracker behind the onset stage, through the same chain body: the envelope (onset,
 * which must agree with the spectral spec as vsyn_rhythm_spec.onset must), then with beat->bpm == 0 the tempogram mean for ac_size 8 s,
 * a copy of the means to the host, vsyn_tempo_from_mean and P per segment, then D.1 to D.5. rows receives the beat frames as uint32
 * words (rows_capacity counts words; F a segment suffice) and seg_rows their counts; bpm_out[S] the tempo the period came from (0.0
 * for a segment without beats by D.0, a refused or a skipped one), rate_out[S] the rate the rows were computed at, refused_out[S] the
 * words of D.0 (each may be NULL). beat = NULL or onset = NULL is refused: the other entries are not rerouted. Synchronous. */
int vsyn_pcm_chain_beats_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                              const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                              const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                              const vsyn_onset_spec* onset, const vsyn_beat_spec* beat, uint32_t num_segments, const uint32_t* in_rates,
                              uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out,
                              uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out,
                              double* refs_out, vsyn_loudness_record* records_out, double* bpm_out, uint32_t* rate_out,
                              uint32_t* refused_out, vsyn_status* status, const char** err);

/* ---- inverse STFT: complex rows, with or without a real mask on them, back to PCM, computed where the rows are ----
 *
 * Input: one segment's rows X[f][k], F rows (time) of n_fft / 2 + 1 complex64 bins, the layout VSYN_SPEC_STFT writes; optionally a
 * float32 mask m[f][k] of the same shape, the layout of VSYN_HPSS_OUT_MASK on VSYN_SPEC_LIN_POWER rows. Output: `length` float32
 * samples. This is librosa.istft(X.T, hop_length=hop_length, win_length=win_length, n_fft=n_fft, window="hann", center=..., length=
 * length) of m * X. librosa is not among the test dependencies and parity with it is not claimed: the contract is the arithmetic
 * below, the device is compared against a float64 model of it (tests/istft_model.py), and the model against torch.istft and a direct
 * inverse DFT (tests/test_istft_cpu.py).
 *
 *  1. Y[f][k] = m[f][k] * X[f][k], one float32 product per component; Y = X without a mask.
 *  2. x_f = irfft(Y_f, n_fft), the 1 / n_fft included; the imaginary parts of bins 0 and n_fft / 2 are not read, as numpy does not
 *     read them. In float32: with M = n_fft / 2, a = Y[k], b = Y[M - k] and (c, s) = (cos, sin)(2 pi k / n_fft) rounded to float32,
 *     Z[k] = (er - (c di + s dr), ei + (c dr - s di)), er = a.re + b.re, ei = a.im - b.im, dr = a.re - b.re, di = a.im + b.im, for
 *     k < M; then log2 M radix-2 Stockham passes over Z (butterfly j of pass Ns: a = in[j], b = in[j + M/2], t = (c b.re - s b.im,
 *     c b.im + s b.re) with (c, s) of angle 2 pi (j mod Ns) / (2 Ns), out[j0] = a + t, out[j0 + Ns] = a - t, j0 = 2 (j - j mod Ns) +
 *     j mod Ns), the forward kernel's passes with conjugated twiddles; z[m] then holds n_fft x_f[2m] and n_fft x_f[2m + 1], and each
 *     is multiplied by 1 / n_fft (exact). Plain products and sums in the order written; nothing is contracted.
 *  3. v_f[j] = w[j] * x_f[j] on the window's support, one float32 product; w is the forward table's window (periodic Hann of
 *     win_length, built in double, rounded to float32, centred in n_fft). Outside the support a frame contributes nothing.
 *  4. y[t] = (sum_f v_f[t + pad - f hop_length]) / W[t], W[t] = sum_f w[t + pad - f hop_length]^2, pad = n_fft / 2 with
 *     VSYN_SPEC_CENTER, else 0, both over the frames whose window support holds t. Both sums are float64, from 0.0, in ascending f
 *     (their terms: the float32 v, and the exact float64 square of the float32 w); the quotient is float64 and is rounded once to
 *     float32. Where W[t] <= FLT_MIN the sum is left undivided (librosa's `tiny` rule). A sample that no frame covers is 0. `length`
 *     shorter than what the frames cover cuts the signal, a longer one appends zeros.
 *  5. Non-finite values. A NaN or an Inf in bin k of row f (the imaginary parts of bins 0 and n_fft / 2 excepted: they are not
 *     read), or in its mask, makes every x_f[j] non-finite and with it exactly the samples under frame f's window support, w[j] = 0
 *     included. Every other sample, segment, length word and byte behind a segment's length keeps its bits.
 *  6. Checks (VSYN_ERR_INVALID before anything runs, the outputs untouched): the spec's n_fft, hop_length and win_length as the
 *     spectral entry points check them (the spec's other fields but VSYN_SPEC_CENTER are not read); n_fft a power of two, any other
 *     refused by name; NULL seg_rows, rows or output; a length above out_plane_stride; out_plane_stride >= 2^32.
 *  7. Not built: the inverse of the direct-DFT path (an n_fft that is no power of two); other windows; a fused single kernel in
 *     which a workgroup owns an output span and recomputes its edge frames; Griffin-Lim and spectral gating, each of which is
 *     one kernel on top of this stage (the phase-vocoder time stretch is built: "phase vocoder").
 *
 * Precision and order. Every frame's arithmetic is its own: nothing of one frame enters another's transform, and step 4 adds in
 * ascending f whatever the grid. No atomics: the result depends on neither the launch geometry nor the segment's place in the batch,
 * the same rows give the same bits. The entry points read rows and mask only: they touch neither stream state, the overlap buffers
 * nor the PCM kept by VSYN_SUBMIT_KEEP_PCM. One handle's inverse-STFT entry points share its frame workspace (rows * n_fft floats,
 * grown on demand). */

/* Samples that `rows` rows cover: hop_length (rows - 1), plus n_fft without VSYN_SPEC_CENTER; 0 for no rows or a refused spec. */
uint64_t vsyn_istft_num_samples(const vsyn_spectral_spec* spec, uint64_t rows);

/* The stage on rows the caller has on the device: d_rows holds the segments' rows back to back, n_fft / 2 + 1 complex64 bins each
 * (8-byte aligned); d_mask (may be NULL) the masks in the same order, one float32 per bin; seg_rows[S] is a HOST array of each
 * segment's row count, lengths[S] a HOST array of each segment's output length (NULL: vsyn_istft_num_samples of its rows). Segment
 * g's samples go to d_pcm_out + g * out_plane_stride, exactly lengths[g] of them and nothing behind them; d_out_frames[g] (may be
 * NULL) receives lengths[g]. Asynchronous on hip_stream. */
int vsyn_istft_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t num_segments, const uint64_t* seg_rows, const float* d_rows,
                      const float* d_mask, const uint64_t* lengths, float* d_pcm_out, uint64_t out_plane_stride, uint32_t* d_out_frames,
                      void* hip_stream, const char** err);

/* ---- PCM effects: the harmonic or the percussive component of the decoded PCM as PCM, computed where the PCM is ----
 *
 * librosa.effects.harmonic(y) / percussive(y) for one segment: y_c = istft(m_c * stft(y)), m_c the soft mask of
 * librosa.decompose.hpss on |stft(y)|. Parity with librosa is not claimed; the contract is the composition below, of stages whose
 * arithmetic their own sections pin, and the stage equals that composition through the public device entry points bit for bit
 * (tests/test_gpu_pcm_effects.py).
 *
 *  1. S = the VSYN_SPEC_LIN_POWER rows, power 1, of the segment's mono downmix ("linear spectra"), with n_fft, hop_length, win_length
 *     of the effect and always centred: 1 + T / hop_length rows for T > 0 samples.
 *  2. m = the VSYN_HPSS_OUT_MASK output of the HPSS stage on S ("HPSS") under effect->hpss (its kernel sizes, component, power and
 *     margins).
 *  3. y_c = the inverse STFT ("inverse STFT") of X = the VSYN_SPEC_STFT rows of the same signal, under the mask m, centred, to
 *     length T. X is computed in the workgroup that inverts it and is never stored; its bits are those VSYN_SPEC_STFT stores.
 *  4. Order in the pipeline: resampler, trim / split, this stage, loudness, peak normalisation and pre-emphasis: those act on the
 *     component, as they would on librosa.effects.harmonic(y). Output: a mono signal of the same frame count.
 *  5. Non-finite samples flow through as the three stages' rules say: a NaN or an Inf sample makes the frames that hold it non-finite,
 *     a NaN in S makes the masks of its median windows NaN, and those make the samples under their frames' supports non-finite.
 *  6. Checks (VSYN_ERR_INVALID before anything runs, outputs untouched): n_fft a power of two in [16, 8192], any other refused by
 *     name; hop_length >= 1; win_length in [1, n_fft]; the hpss spec as the HPSS stage checks it, and its output must be
 *     VSYN_HPSS_OUT_COMPONENT: the mask and the median are not signals.
 *  7. Not built: the effect in front of the spectral, pitch, descriptor and loudness row entries (the steps are shared, so this is
 *     the natural follow-up); both components from one call; the residual (time stretch and pitch shift are built: "PCM
 *     stretch").
 * The entry points read PCM only, and share the handle's spectral, HPSS and inverse-STFT workspaces with those stages' entries. */
typedef struct vsyn_pcm_effect { /* 56 bytes */
  uint32_t n_fft;      /* a power of two in [16, 8192]; librosa's default is 2048 */
  uint32_t hop_length; /* >= 1; n_fft / 4 */
  uint32_t win_length; /* 1 .. n_fft; n_fft */
  uint32_t reserved;   /* 0 */
  vsyn_spectral_hpss hpss; /* output must be VSYN_HPSS_OUT_COMPONENT */
} vsyn_pcm_effect;

/* The stage alone on PCM the caller has on the device: d_pcm planar [S][channels][plane_stride] float32, frames[S] a HOST array of
 * each segment's frame count (at most both strides). Segment g's component goes to d_pcm_out + g * out_plane_stride, exactly
 * frames[g] samples and nothing behind them; d_out_frames[g] (may be NULL) receives frames[g]. Asynchronous on hip_stream. */
int vsyn_pcm_hpss_device(vsyn_handle* h, const vsyn_pcm_effect* effect, uint32_t num_segments, const uint64_t* frames, const float* d_pcm,
                         uint64_t plane_stride, uint32_t channels, float* d_pcm_out, uint64_t out_plane_stride, uint32_t* d_out_frames,
                         void* hip_stream, const char** err);

/* vsyn_pcm_chain_host with the effect between the gate and the loudness step, through the same chain body, without PCM or rows
 * leaving the device: out receives ONE plane per segment. effect = NULL is that entry, bit for bit. Synchronous. */
int vsyn_pcm_chain_effects_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond, uint32_t num_segments, const uint32_t* in_rates,
                                uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out,
                                uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                vsyn_loudness_record* records_out, const char** err);

/* ---- phase vocoder: complex rows to the complex rows of the time-stretched signal, computed where the rows are ----
 *
 * Input: one segment's rows X[f][k], F rows (time) of nb = n_fft / 2 + 1 complex64 bins, the layout VSYN_SPEC_STFT writes, and a rate
 * per SEGMENT, a finite double above 0 (above 1 shortens). Output: F_out rows of the same layout. This is librosa.phase_vocoder(X.T,
 * rate=rate, hop_length=hop_length, n_fft=n_fft). librosa is not among the test dependencies and parity with it is not claimed: the
 * contract is the arithmetic below, the device is compared against a float64 model of it fed the same float32 rows
 * (tests/pv_model.py), and the model against a literal transcription of librosa's sequential loop (tests/test_pv_cpu.py).
 *
 *  1. F_out = ceil(F / rate), one float64 quotient: len(numpy.arange(0, F, rate)); F = 0 gives no rows. Output row t sits at s_t =
 *     t * rate (one float64 product), i_t = floor(s_t), alpha_t = s_t - i_t. Rows of index >= F read as +0 + 0i (librosa pads two).
 *  2. Per input row and bin, in float64 from the float32 components: A = atan2((double)im, (double)re), G = sqrt(re * re + im * im).
 *     C99's signed zeros are part of the contract: atan2(+0, -0) = pi, atan2(-0, -0) = -pi, atan2(+-0, +0) = +-0, so that a silent
 *     stretch in the middle of a file leaves the phase of what follows where it was.
 *  3. phi_k = hop_length * (k * (1.0 / (n_fft * (1.0 / (2 pi))))), float64 on the host (numpy's rfftfreq expression); d = A[i_t + 1][k]
 *     - A[i_t][k] - phi_k; inc_t = phi_k + (d - 2 pi * rint(d / (2 pi))), rint to even, 2 pi the double nearest it.
 *  4. acc_0 = A[0][k] and acc_{t+1} = acc_t + inc_t, in a FIXED blocked order: output rows go in blocks of VSYN_PV_BLOCK = 64 rows of
 *     the segment. A block's sum is ((0.0 + inc_b0) + inc_b0+1) + ...; the carry of block b is ((A[0][k] + sum_0) + sum_1) + ... +
 *     sum_{b-1}; inside a block acc starts at the carry and adds inc_t in ascending t. The block size is a constant of the contract:
 *     nothing depends on the grid, the tile of bins or the segment's place in the batch.
 *  5. out[t][k] = ((float)(m cos(acc_t)), (float)(m sin(acc_t))), m = (1 - alpha_t) G[i_t][k] + alpha_t G[i_t + 1][k], everything in
 *     float64 with one rounding per component. Plain products and sums in the order written; nothing is contracted.
 *  6. Non-finite values, per bin k (other bins, and other segments, keep their bits). A NaN component in X[f][k] makes A and G of
 *     that row NaN: m_t is NaN for i_t in {f - 1, f} (alpha_t = 0 included: 0 * NaN), inc_t is NaN for the same t, and acc stays NaN
 *     behind the first of them. So with t0 the first t whose i_t is f - 1 or f, out[t][k] is NaN for every t >= t0; f = 0 has t0 = 0
 *     (acc_0 itself). At a rate above 2 the walk can step over both f - 1 and f: then no t0 exists and nothing changes. An Inf
 *     component has a finite angle and G = Inf: exactly the rows with i_t in {f - 1, f} are non-finite (+-Inf, or NaN from 0 * Inf
 *     where alpha_t = 0). The rows in front of t0 keep their bits; the rows behind the last of them are finite, but carry the
 *     phase that the angle of the Inf (a multiple of pi / 4) left in acc, so their bits may differ from the clean run's.
 *  7. Checks (VSYN_ERR_INVALID before anything runs, the outputs untouched): n_fft a power of two in [16, 8192] and hop_length >= 1
 *     as the inverse STFT checks them (win_length and the spec's other fields are not read); a rate that is not finite or <= 0; a
 *     segment of more than 2^30 - 1 rows in or out; NULL seg_rows, rates, rows or output; more than 65535 segments.
 *  8. Not built: fusing the emit kernel into the inverse STFT's frame kernel (the stretched rows pass through memory); phase locking
 *     and other vocoder variants; an n_fft that is no power of two.
 *
 * Precision and order: no atomics, the same rows and rate give the same bits whatever the batch. The entry reads the rows only. One
 * handle's calls share its block-sum workspace (F_out / 64 rows of nb float64, grown on demand). */
#define VSYN_PV_BLOCK 64u

/* F_out of step 1: host arithmetic, no device. 0 for a rate the stage refuses. */
uint64_t vsyn_pv_num_rows(uint64_t rows, double rate);

/* The stage on rows the caller has on the device: d_rows holds the segments' rows back to back, nb complex64 bins each (8-byte
 * aligned); seg_rows[S] and rates[S] are HOST arrays. Segment g's F_out rows go to d_rows_out back to back in the same order (the
 * caller sizes it from vsyn_pv_num_rows; it must not overlap d_rows); seg_rows_out[S] (HOST, may be NULL) receives each F_out.
 * Of spec only n_fft and hop_length are read. Asynchronous on hip_stream. */
int vsyn_phase_vocoder_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t num_segments, const uint64_t* seg_rows, const double* rates,
                              const float* d_rows, float* d_rows_out, uint64_t* seg_rows_out, void* hip_stream, const char** err);

/* ---- PCM stretch: the decoded PCM time-stretched, or pitch-shifted, as PCM, computed where the PCM is ----
 *
 * librosa.effects.time_stretch(y, rate=rate) for one segment, and with a resampling behind it librosa.effects.pitch_shift. Parity
 * with librosa is not claimed; the contract is the composition below, of stages whose arithmetic their own sections pin, and the
 * stage equals that composition through the public device entry points bit for bit (tests/test_gpu_pcm_stretch.py). Per segment of
 * T frames, always centred, on the mono downmix:
 *
 *  1. X = the VSYN_SPEC_STFT rows ("linear spectra") with the stage's n_fft, hop_length, win_length.
 *  2. Y = the phase vocoder's rows ("phase vocoder") of X at the segment's rate.
 *  3. y = the inverse STFT ("inverse STFT") of Y without a mask, to length L = vsyn_stretch_num_samples(T, rate) = nearbyint(T /
 *     rate), ties to even: Python's int(round(T / rate)).
 *  4. With shift_to_hz != 0: y resampled from shift_from_hz[g] to shift_to_hz ("resampling"), vsyn_resample_num_frames of L frames.
 *  5. With VSYN_STRETCH_FIX_LENGTH: exactly T samples, the first T of what step 3 or 4 left, or all of it followed by zeros.
 *  6. pitch_shift by n_steps of bins_per_octave is this stage with rate = 2^(-n_steps / bins_per_octave), shift_to_hz = sr,
 *     shift_from_hz = rint(sr / rate) and the length fixed. ONE DIVERGENCE from librosa: it resamples from the non-integer sr / rate,
 *     this stage from that rate rounded to whole Hz, because its resampler is resample_poly's arithmetic on integer rates. That moves
 *     the pitch by at most 0.5 / (sr / rate) relative. The pair must pass the resampler's check max(up, down) <= VSYN_RESAMPLE_MAX_M.
 *  7. Order in the pipeline: resampler, trim / split, this stage, loudness, peak normalisation and pre-emphasis. This is the one
 *     stage behind the gate that changes the frame count: the steps behind it see the stage's frames.
 *  8. Non-finite samples flow through as the stages' rules say.
 *  9. Checks (VSYN_ERR_INVALID before anything runs, outputs untouched): the framing as "PCM effects" checks it; unknown options; a
 *     non-zero reserved; a rate that is not finite or <= 0; with a shift a NULL shift_from_hz, a from-rate of 0 or a pair the
 *     resampler refuses, by name; an out_plane_stride below a segment's delivered frames.
 * 10. Not built: the stretch in front of the spectral, pitch, descriptor and rhythm row entries; the stretch composed with the HPSS
 *     effect; librosa's non-integer resampling rate; fusing the vocoder into the inverse frame kernel.
 * The entry points read PCM only, and share the handle's spectral, phase-vocoder and inverse-STFT workspaces with those stages'
 * entries; the resampler's workspace is the stage's own. */
#define VSYN_STRETCH_FIX_LENGTH 1u /* cut or zero-pad each output to its input's frames */
typedef struct vsyn_pcm_stretch { /* 24 bytes */
  uint32_t n_fft;       /* a power of two in [16, 8192]; librosa's default is 2048 */
  uint32_t hop_length;  /* >= 1; n_fft / 4 */
  uint32_t win_length;  /* 1 .. n_fft; n_fft */
  uint32_t options;     /* VSYN_STRETCH_FIX_LENGTH */
  uint32_t shift_to_hz; /* 0: time stretch only. Else: behind the stretch, each segment is resampled from shift_from_hz[g] to this rate */
  uint32_t reserved;    /* 0 */
} vsyn_pcm_stretch;

/* L of step 3: host arithmetic, no device. 0 for a rate the stage refuses. */
uint64_t vsyn_stretch_num_samples(uint64_t frames, double rate);

/* The stage alone on PCM the caller has on the device: d_pcm planar [S][channels][plane_stride] float32; frames[S], rates[S] and
 * shift_from_hz[S] (NULL without a shift) are HOST arrays. Segment g's samples go to d_pcm_out + g * out_plane_stride, exactly its
 * delivered frames (step 3, 4 or 5) and nothing behind them; d_out_frames[g] (may be NULL) receives that count. Asynchronous on
 * hip_stream. */
int vsyn_pcm_stretch_device(vsyn_handle* h, const vsyn_pcm_stretch* stretch, uint32_t num_segments, const uint64_t* frames, const double* rates,
                            const uint32_t* shift_from_hz, const float* d_pcm, uint64_t plane_stride, uint32_t channels, float* d_pcm_out,
                            uint64_t out_plane_stride, uint32_t* d_out_frames, void* hip_stream, const char** err);

/* vsyn_pcm_chain_effects_host with the stretch stage in the effect's slot, through the same chain body: stretch_rates[S] and
 * shift_from_hz[S] (NULL without a shift) are HOST arrays per segment. stretch = NULL is that entry, bit for bit; a stretch and an
 * effect in one call are refused by name. frames_out[g] receives the stage's delivered frames, and the loudness and conditioning
 * steps see those. out_stride_frames must hold the largest of each segment's frames in front of the gate, stretched, resampled and
 * delivered (a gate only shortens, and every one of them is monotone in the frames): a call with out = NULL returns that need in
 * frames_out instead, as every chain entry's size query does. Synchronous. */
int vsyn_pcm_chain_stretch_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                const vsyn_pcm_stretch* stretch, const double* stretch_rates, const uint32_t* shift_from_hz,
                                const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond, uint32_t num_segments, const uint32_t* in_rates,
                                uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out,
                                uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                vsyn_loudness_record* records_out, const char** err);

#ifdef __cplusplus
}
#endif
#endif /* VORBIS_SYNTH_HIP_H_ */
