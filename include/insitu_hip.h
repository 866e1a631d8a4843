/*
 * insitu_hip.h -- C ABI of libinsitu_hip.so, the MI355X-native replacement for the
 * native half of scenery-insitu's distributed VDI volume-rendering path.
 *
 * In the reference, the Kotlin host (DistributedVolumeRenderer.kt / DistributedVolumes.kt)
 * renders sub-VDIs with Vulkan compute shaders, reads them back to host ByteBuffers and
 * hands them to external native code (OpenFPM's InVis.cpp, README.md:19) through
 *   external fun distributeVDIs(...)        DistributedVolumeRenderer.kt:112, DistributedVolumes.kt:136-137
 *   external fun gatherCompositedVDIs(...)  DistributedVolumeRenderer.kt:113, DistributedVolumes.kt:138-139
 * which run MPI_Alltoall / MPI_Gather and call back into Kotlin (compositeVDIs :684,
 * uploadForCompositing DistributedVolumes.kt:945, streamImage :726).
 *
 * Here the whole frame stays on the GPU: insitu_render replaces the Vulkan dispatch of
 * VDIGenerator.comp+AccumulateVDI.comp (or VolumeRaycaster.comp+AccumulatePlainImage.comp),
 * insitu_exchange replaces distributeVDIs' MPI_Alltoall (RCCL over xGMI, device buffers),
 * insitu_composite replaces the compositor dispatch (PlainImageCompositor.comp, or the VDI
 * flatten of VDIGenerator.comp:147-185 in VDICompositor.comp:58-91 order), and
 * insitu_gather replaces gatherCompositedVDIs' MPI_Gather.  insitu_view_bind / insitu_view_render
 * render the last completed VDI from any other camera (the consumer the VDI exists for: the
 * reference's EfficientVDIRaycast.comp).  The reference-shaped entry
 * points at the bottom keep the exact Kotlin argument lists for a JNI shim
 * (INTEGRATION.md).
 *
 * Conventions: 0 = success, negative = error (insitu_last_error() has the text).  A context
 * is owned by one thread.  Calls are ordered on the context's HIP stream; insitu_gather,
 * insitu_read and insitu_synchronize block.  Matrices are column-major float[16] (GLSL/JOML).
 */
#ifndef INSITU_HIP_H
#define INSITU_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INSITU_ABI_VERSION 12
#define INSITU_COMM_ID_BYTES 128

typedef struct insitu_ctx insitu_ctx;
/* In-process rank group: the contexts of all ranks live in one process (on any devices) and the
 * exchange/gather copy device to device instead of RCCL.  Used to run the multi-rank data path
 * on one GPU (RCCL refuses two ranks per device); each stage must then be called for every rank
 * before the next stage starts (render all, exchange all, composite all, gather all). */
typedef struct insitu_local_group insitu_local_group;

enum insitu_mode {
    INSITU_MODE_PLAIN = 0, /* DistributedVolumeRenderer.kt: generateVDIs = false (:78)  */
    INSITU_MODE_VDI = 1    /* DistributedVolumes.kt:      generateVDIs = true  (:88)  */
};

enum insitu_dtype { INSITU_U8 = 0, INSITU_U16 = 1, INSITU_F32 = 2 };

enum insitu_buf {
    INSITU_BUF_VDI_COLOR = 0,   /* brick `slot`: (S,H,W) rgba32f, reference layout (DistributedVolumes.kt:349-358) */
    INSITU_BUF_VDI_DEPTH = 1,   /* brick `slot`: (2S,H,W) r32f (DistributedVolumes.kt:360-368)                    */
    INSITU_BUF_OCTREE = 2,      /* brick `slot`: (W/8,H/8,S) r32ui OctreeCells (DistributedVolumes.kt:342,370-374)  */
    INSITU_BUF_PASSES = 3,      /* brick `slot`: H*W uint8 raymarch passes per pixel (needs keep_passes)          */
    INSITU_BUF_PLAIN_COLOR = 4, /* brick `slot`: (dim0,dim1) rgba8 OutputSubVDIColor (DistributedVolumeRenderer.kt:214) */
    INSITU_BUF_PLAIN_DEPTH = 5, /* brick `slot`: (dim0,dim1) rgba8 OutputSubVDIDepth (EncodeFloatRGBA(tnear))      */
    INSITU_BUF_STRIP = 6,       /* this rank's composited strip, rgba8 (VDI: H x W/P row-major; plain: rows x dim0) */
    INSITU_BUF_IMAGE = 7,       /* root: gathered full image rgba8, row-major (H,W) / (dim1,dim0)                  */
    /* composite_vdi contexts (VDICompositor.comp output, DistributedVolumes.kt:423-431):              */
    INSITU_BUF_COMPOSITED_COLOR = 8,  /* this rank's strip: (S_out,H,W/P) rgba32f CompositedVDIColor     */
    INSITU_BUF_COMPOSITED_DEPTH = 9,  /* this rank's strip: (2S_out,H,W/P) r32f CompositedVDIDepth       */
    INSITU_BUF_GATHERED_COLOR = 10,   /* root: (S_out,H,W) rgba32f, the gathered composited VDI          */
    INSITU_BUF_GATHERED_DEPTH = 11,   /* root: (2S_out,H,W) r32f                                         */
    INSITU_BUF_COMPOSITE_PASSES = 12, /* this rank's strip: H*(W/P) uint8 compositor search passes      */
    /* VDI mode, after insitu_exchange (or insitu_distribute_vdis): the set this rank composites, in the
     * reference layout -- nranks * bricks source-major blocks of (S,H,W/P) rgba32f / (2S,H,W/P) r32f,
     * empty slots zero: what allToAllColorPointer holds and uploadForCompositing receives
     * (DistributedVolumes.kt:945), dumped as SetOfVDI{n}_ndc_col / _ndc_depth (:974-975)        */
    INSITU_BUF_RECEIVED_COLOR = 13,
    INSITU_BUF_RECEIVED_DEPTH = 14,
    /* after insitu_view_render: the view of the bound VDI from the last viewing camera */
    INSITU_BUF_VIEW_COLOR = 15,  /* (out_h,out_w) rgba32f, the front-to-back accumulator           */
    INSITU_BUF_VIEW_IMAGE = 16   /* (out_h,out_w) rgba8                                            */
};

/* What insitu_view_bind takes its VDI from. */
enum insitu_view_source {
    INSITU_VIEW_GATHERED = 0, /* root of a composite_vdi context: the gathered composited VDI (W,H,S_out) */
    INSITU_VIEW_BRICK = 1,    /* brick `slot`'s sub-VDI (W,H,S)                                             */
    INSITU_VIEW_MERGED = 2    /* all sub-VDIs this rank rendered, merged per pixel by start depth (W,H,S_m);
                                 `slot` must be 0                                   */
};

/* Colour precision of a packed VDI stream (insitu_view_pack); the depths are float32 in both. */
enum insitu_pack_format {
    INSITU_PACK_FLOAT = 0, /* rgba32f: the bound VDI exactly, 24 bytes per stored entry                     */
    INSITU_PACK_HALF = 1   /* rgba16f, round to nearest even (numpy's astype(float16)): 16 bytes per entry  */
};

typedef struct insitu_config {
    int rank;              /* DistributedVolumes.rank (:104)                               */
    int nranks;            /* commSize (:103)                                              */
    int device;            /* nodeRank -> scenery.Renderer.DeviceId (:450-451)             */
    int width, height;     /* window W,H; plain mode: texture dims (dim0, dim1)             */
    int max_supersegments; /* maxSupersegments S (DistributedVolumes.kt:99); plain: 1      */
    int mode;              /* enum insitu_mode                                              */
    int bricks_per_rank;   /* bricks (volumes) rendered by this rank; each is one sub-VDI   */
    const void* comm_id;   /* INSITU_COMM_ID_BYTES from insitu_comm_id() on rank 0; NULL if nranks == 1 */
    void* stream;          /* hipStream_t to run on; NULL -> the context creates one        */
    int keep_passes;       /* record per-pixel raymarch pass counts (INSITU_BUF_PASSES)     */
    int sample_cache_mb;   /* VDI mode: HBM for the per-sample raymarch cache, MiB; 0 = default
                              (512 B per pixel per brick at first, grown after a frame whose rays did
                              not fit to 1.25x that frame's demand, at most 45 % of the HBM free at
                              create), > 0 = fixed size, < 0 = off */
    int composite_vdi;     /* VDI mode: 0 = insitu_composite flattens the merged lists to RGBA
                              (accumulateSupseg, VDIGenerator.comp:147-185); 1 = VDICompositor.comp:
                              re-supersegment them into a composited VDI of max_output_supersegments
                              per pixel, gathered to rank 0 (DistributedVolumes.kt:903)         */
    int max_output_supersegments; /* maxOutputSupersegments S_out (DistributedVolumes.kt:100); 0 -> S */
    insitu_local_group* local_group; /* non-NULL: in-process rank group instead of RCCL (comm_id unused) */
    int faithful;          /* bit mask of enum insitu_faithful: reproduce a reference quirk instead of the
                              default (corrected) behaviour, for parity with the shaders as written */
    int merge_bricks;      /* VDI mode: 1 = the rank's bricks are the volumes of ONE sub-VDI, as
                              VDIGenerator.comp renders all of a rank's grids ($repeat over volumes,
                              :333-347; several grids per compute partner, DistributedVolumeRenderer.kt:57-63);
                              0 = every brick is its own sub-VDI (a virtual rank).  Merged volumes run
                              the threshold search through the per-sample cache too (64-byte slots that
                              carry each sample's step index)                   */
} insitu_config;

/* Reference quirks (default off: the corrected behaviour). */
enum insitu_faithful {
    /* VDICompositor.comp:204: ndc_x from gl_GlobalInvocationID.x, the strip-LOCAL column, over the
     * full window width (default: the pixel's global column; the two agree on rank 0 only) */
    INSITU_FAITHFUL_COMPOSITOR_NDC_X = 1,
    /* PlainImageCompositor.comp:43: numProcesses = imageSize.r / imageSize.g = dim0 * nranks / dim1
     * (default: every list; the two agree for square windows) */
    INSITU_FAITHFUL_PLAIN_NUM_PROCESSES = 2
};

typedef struct insitu_camera {
    float view[16];     /* LightParameters.ViewMatrices[0]                                 */
    float proj[16];     /* LightParameters.ProjectionMatrix (Vulkan-corrected, DistributedVolumes.kt:67-79) */
    float inv_view[16]; /* InverseViewMatrices[0]  (used when has_inverses != 0)           */
    float inv_proj[16]; /* InverseProjectionMatrix (used when has_inverses != 0)           */
    int has_inverses;   /* 0 -> computed here in double precision                          */
    float nw;           /* VolumeManager shaderProperties["nw"] (DistributedVolumes.kt:713) */
    float fwnw;         /* plain mode only (VolumeRaycaster.comp:133-139)                   */
    float tmax;         /* getMaxDepth(): 1.0 = no opaque geometry                          */
} insitu_camera;

typedef struct insitu_stats {
    float ms_render, ms_exchange, ms_composite, ms_gather; /* HIP-event times of the last frame */
    float ms_sample, ms_search;  /* VDI render split: first-pass sampling kernel / threshold-search kernel */
    /* VDI render counters of the last frame (all local bricks): */
    long long rays_searched;     /* rays queued for the threshold search after the first pass        */
    long long rays_uncached;     /* rays that hit a brick but got no per-sample cache space: searched
                                    by re-sampling the brick every pass (same results, slower)       */
    long long cache_bytes;       /* capacity of the per-sample cache                                 */
    long long exchange_bytes;    /* bytes this rank sent to peers in the last exchange (VDI mode:
                                    the compact messages -- counts, tile offsets, stored entries)     */
    long long exchange_entries;  /* supersegment entries this rank sent to peers (VDI mode)          */
    float ms_compact;            /* VDI mode, nranks > 1: packing the stored supersegments bound for
                                    the peers (counted in ms_exchange, not in ms_render)              */
    float ms_exchange_sync;      /* VDI mode, nranks > 1: GPU idle time of the exchange's host round trip
                                    (the receive sizes reach the host before the payload is enqueued) */
    long long cache_demand_bytes; /* per-sample cache the last render's rays asked for (fits when
                                    <= cache_bytes; a default-sized cache grows to it)               */
    int search_regroups;         /* VDI mode: waves of the threshold search that re-formed their lanes into
                                    deeper search trees once the queue was drained (INSITU_OPT_REGROUP) */
    float ms_image_d2h;          /* root: copy of the final image to the host buffer of insitu_gather
                                    (what streamImage receives, DistributedVolumeRenderer.kt:726); 0 when
                                    no host buffer was passed                                          */
    float ms_latency;            /* render start to the image on the host (or the gather's end) of the
                                    frame: with insitu_frame_pipelined it spans the next frame's start   */
    int pipelined;               /* 1: the frame was rendered by insitu_frame_pipelined (its render starts
                                    at its trigger: its prepare was queued ahead of it)   */
    float ms_ingest;             /* GPU time of the last batch of insitu_set_brick re-ingests (the bricks set
                                    between two renders; 0 until one has completed)                     */
    float ms_view;               /* GPU time of the last insitu_view_render's kernel (0 until one has run)  */
    float ms_pack;               /* GPU time of the kernels of the last insitu_view_pack or insitu_view_bind_packed
                                    (offsets, copy; the copies to and from the host are not in it)           */
    int view_slots;              /* slots per pixel S of the bound VDI, whatever bound it (0: none bound)       */
    long long view_overlaps;     /* merged binds: adjacent entries of the bound lists whose next start depth lies
                                    before the previous end (bricks that overlap in space; the viewer trusts a
                                    list not to); 0 for the binds of one VDI                                   */
    float ms_view_bind;          /* GPU time of the kernels of the last bind (uploads and readbacks not in it)  */
    long long view_entries;      /* stored entries E of the bound VDI, the sum of its counts, whatever bound it and in
                                    either layout (0: none bound)                                                */
    long long view_bytes;        /* device bytes the bound VDI's view layout uses (not what the grow-only buffers
                                    hold), tiles = ceil(W/8)*ceil(H/8), nblocks = ceil(W*H/256):
                                      dense:   24*W*H*S + W*H + tiles
                                      compact: 24*max(E,1) + 3*W*H + 8*nblocks + tiles                           */
    int view_compact;            /* 1: the bound VDI is in the compact layout (INSITU_OPT_VIEW_COMPACT at its bind) */
} insitu_stats;

/* Tuning and diagnostics options (insitu_set_option); the defaults are the measured optimum. */
enum insitu_option {
    INSITU_OPT_EXACT_SEARCH = 0,   /* 1: every supersegment decision by the exact contract path
                                      (default 0: filtered decisions -- identical results)         */
    INSITU_OPT_SEARCH_DEPTH = 1,   /* 0 = from the queue length; 1..6 tree levels per replay round */
    INSITU_OPT_LONG_SAMPLES = 2,   /* rays with at least this many samples are searched first      */
    INSITU_OPT_ROUND_BATCH = 3,    /* 1..64: lanes that end a search round together                */
    INSITU_OPT_SEARCH_OVERSUB = 4, /* 1..64: queue length x group size per resident search lane    */
    INSITU_OPT_TILE_ORDER = 5,     /* 1 (default): sampling tiles longest-first; 0: plain XCD order */
    /* 6 and 7 (ABI 6: the fused generator modes, measured slower and removed in ABI 7) are rejected */
    INSITU_OPT_SUPER_TILE = 8,     /* 1, 2 or 4: the longest-first order sorts super-tiles of this many
                                      tiles per edge, a super-tile's tiles kept together (one XCD's L2) */
    INSITU_OPT_REGROUP = 9,        /* 1 (default): once the search queue is drained, a wave deals its lanes
                                      out again so the rays left get deeper search trees; 0: off        */
    INSITU_OPT_EXACT_TILE_KEYS = 10, /* 1: the longest-first order keys a tile by all 64 of its rays;
                                      0 (default): by 16 of them (frames that size the cache: all)      */
    /* insitu_frame_pipelined: when frame k+1's first pass (the sampling kernel) may start beside frame k */
    INSITU_OPT_PIPE_TRIGGER = 11,  /* 0: after frame k's threshold search; 1: when frame k's search queue is
                                      drained (its tail: the rays in flight); 2 (default): at once (after
                                      frame k's first pass, sharing the GPU with its whole search, whose
                                      grid leaves it wave slots: INSITU_OPT_PIPE_SEARCH_RAYS)              */
    INSITU_OPT_PIPE_OVERSUB = 12,  /* 1..64: INSITU_OPT_SEARCH_OVERSUB of pipelined frames (default 3; their
                                      search shares the GPU with the next frame's first pass, so fewer
                                      speculative tree lanes pay: DESIGN.md 5.1)                          */
    INSITU_OPT_PIPE_SEARCH_RAYS = 13, /* pipelined frames: queued rays per searching block of the threshold
                                      search, which then keeps one to two blocks per CU and leaves the other
                                      wave slots to the next frame's first pass (default 2048; 0 = the full
                                      persistent grid, as unpipelined frames)                              */
    INSITU_OPT_VIEW_SKIP = 14,     /* insitu_view_render: 1 (default): an 8x8 tile of lists whose largest count
                                      is 0 is stepped over in one step; 0: every cell is walked -- identical
                                      results                                                */
    INSITU_OPT_VIEW_COMPACT = 15   /* the view layout of the VDIs bound from now on (every insitu_view_bind* call):
                                      0 (default): dense, S slots per pixel; 1: compact, the stored entries alone
                                      behind a 3-byte index per pixel -- the same renders and packed streams bit
                                      for bit, less memory.  Takes effect at the next bind: a bound
                                      VDI keeps its layout (insitu_stats.view_compact)                            */
};

int insitu_abi_version(void);
/* ncclUniqueId for a multi-rank context; call on rank 0 and broadcast the bytes. */
int insitu_comm_id(void* out, size_t cap);
int insitu_create(const insitu_config* cfg, insitu_ctx** out);
int insitu_local_group_create(int nranks, insitu_local_group** out);
void insitu_local_group_destroy(insitu_local_group* g);
void insitu_destroy(insitu_ctx* ctx);
/* last error of ctx, or of the last failed insitu_create when ctx == NULL */
const char* insitu_last_error(const insitu_ctx* ctx);

/* Brick upload: replaces addVolume/updateVolume (DistributedVolumes.kt:147-250) and
 * updateData (DistributedVolumeRenderer.kt:136-160).  data is x-fastest dims[0]*dims[1]*dims[2]
 * voxels; data_on_device != 0 means `data` is a device pointer (in-situ zero-copy source, read
 * in place on the context's stream: the work that produced it must be complete, or run on
 * cfg.stream).  model = world matrix of the volume (position, pixelToWorldRatio, origin). */
int insitu_set_brick(insitu_ctx* ctx, int slot, const void* data, int dtype, const int dims[3],
                     const float model[16], int data_on_device);
/* Transfer function (alpha LUT), colour map (rgba LUT) and converter (display range):
 * raw = normalised_voxel * conv_scale + conv_offset, normalised_voxel = v/255, v/65535 or v. */
int insitu_set_transfer(insitu_ctx* ctx, const float* tf, int n_tf, const float* cmap_rgba, int n_cm,
                        float conv_scale, float conv_offset);

/* Camera of the frame (the VDI metadata's view/projection; DistributedVolumes.kt:718-723).
 * insitu_render sets it too; the host-buffer path needs it before insitu_distribute_vdis. */
int insitu_set_camera(insitu_ctx* ctx, const insitu_camera* cam);
int insitu_render(insitu_ctx* ctx, const insitu_camera* cam);   /* all local bricks        */
int insitu_exchange(insitu_ctx* ctx);                          /* screen-strip all-to-all */
int insitu_composite(insitu_ctx* ctx);                         /* sort-last merge of strip */
/* Gather the strips on rank 0.  Root copies the (H,W) rgba8 image to host_out when non-NULL
 * (cap >= W*H*4); other ranks ignore host_out. */
int insitu_gather(insitu_ctx* ctx, void* host_out, size_t cap);
int insitu_frame(insitu_ctx* ctx, const insitu_camera* cam, void* host_out, size_t cap);
/* Pipelined frames, the reference's own loop (DistributedVolumeRenderer.kt:530-542, 577, 602-603: the
 * composite it reads is one frame stale): enqueue frame k's render (camera `cam`) and, while it runs, complete
 * frame k-1 -- exchange, composite, gather, the root's image to host_out -- and return when that is done, with
 * *done_frame = k-1 (-1 for the first call; frames count from 0 per context).  Frame k's first pass runs on
 * a second stream and starts in frame k-1's search tail (INSITU_OPT_PIPE_TRIGGER), so the GPU does not idle
 * between frames.  insitu_read / insitu_read_region / insitu_get_stats / insitu_pass_stats then describe
 * frame k-1.  The second frame's buffers are allocated at the first call (VDI mode, sample cache on, not
 * with a local group).  insitu_set_brick between calls is ordered before the next render; the unpipelined
 * stage calls fail while a frame is in flight. */
int insitu_frame_pipelined(insitu_ctx* ctx, const insitu_camera* cam, void* host_out, size_t cap,
                           long long* done_frame);
/* Complete the frame in flight (as insitu_frame_pipelined's second half); *done_frame = its index, or -1
 * when none was in flight. */
int insitu_pipeline_flush(insitu_ctx* ctx, void* host_out, size_t cap, long long* done_frame);
int insitu_synchronize(insitu_ctx* ctx);
/* Copy a buffer to host in the reference layout (enum insitu_buf). */
int insitu_read(insitu_ctx* ctx, int which, int slot, void* host_out, size_t cap);
size_t insitu_buffer_bytes(const insitu_ctx* ctx, int which);
/* Columns [x0, x1) of brick `slot`'s VDI in the reference layout: INSITU_BUF_VDI_COLOR (x1-x0, H, S)
 * rgba32f, INSITU_BUF_VDI_DEPTH (x1-x0, H, 2S) r32f (x slowest, as (S,H,W) images), or
 * INSITU_BUF_PASSES (H, x1-x0) uint8 -- parity checks of frames too large to read whole. */
int insitu_read_region(insitu_ctx* ctx, int which, int slot, int x0, int x1, void* host_out, size_t cap);
/* ---- novel-view rendering of a VDI ----
 * insitu_view_bind takes a snapshot of a VDI of the last completed frame (enum insitu_view_source; between
 * insitu_frame_pipelined calls the completed frame, as insitu_read) with that frame's camera as the generating
 * camera, and blocks until the snapshot is built: later frames, pipelined ones included, do not disturb it.
 * INSITU_VIEW_GATHERED needs a composite_vdi context, rank 0 and a gathered frame; INSITU_VIEW_BRICK a rendered
 * frame and 0 <= slot < the context's sub-VDIs.  INSITU_VIEW_MERGED (slot 0) binds all of the rank's sub-VDIs of
 * that frame as one VDI: per pixel their lists merged by start depth, the lowest slot first on a tie, as the
 * flatten compositor walks them (VDICompositor.comp:58-91), every entry copied bit for bit.  The bound VDI has
 * S_m = max(1, the longest merged list) slots (insitu_stats.view_slots); more than 255 is rejected with -1.
 * With one sub-VDI (one brick, merge_bricks) it is INSITU_VIEW_BRICK of slot 0; with nranks > 1 it merges the
 * rank's own bricks only, and insitu_view_gather_merged (below) then merges the ranks' bound VDIs on rank 0.
 * A failed insitu_view_bind* call leaves no VDI bound -- whichever of them it is, and wherever it fails. */
int insitu_view_bind(insitu_ctx* ctx, int source, int slot);
/* The same from host memory: a VDI in the reference layout -- colour (W,H,S,4) rgba32f and depth (W,H,2S) r32f, x
 * slowest, as the dumps hold it (vdi_io.read_vdi) -- with the camera that generated it.  W, H and S (1..255) need
 * not be the context's.  A list ends before its first entry whose start depth is 0; the entries before it are
 * trusted to be ordered by depth and not to overlap, as the generator and the compositor write them. */
int insitu_view_bind_host(insitu_ctx* ctx, const void* color, const void* depth, int W, int H, int S,
                          const insitu_camera* gen_cam);
/* The merged bind from host memory: n (1..32) such VDIs of one W, H, S and one generating camera -- the per-rank
 * dumps of a frame, say (DistributedVolumes.kt:848-849) -- merged as INSITU_VIEW_MERGED merges, colors[j] / depths[j]
 * taking the place of slot j.  n = 1 is insitu_view_bind_host. */
int insitu_view_bind_host_set(insitu_ctx* ctx, const void* const* colors, const void* const* depths, int n, int W,
                              int H, int S, const insitu_camera* gen_cam);
/* Render the bound VDI from `cam` at out_w x out_h and block until it is done.  host_out non-NULL: receives the
 * (out_h,out_w) rgba8 image (cap >= out_w*out_h*4).  INSITU_BUF_VIEW_COLOR / INSITU_BUF_VIEW_IMAGE then hold the
 * rgba32f accumulator and the image (insitu_read, insitu_buffer_bytes).  Only cam's view and projection (and its
 * inverses) are used. */
int insitu_view_render(insitu_ctx* ctx, const insitu_camera* cam, int out_w, int out_h, void* host_out, size_t cap);
/* ---- the packed VDI stream ----
 * What stands in for the compacted, compressed VDI the reference publishes to a remote viewer as one message
 * (VolumeFromFileExample.kt:907-1030: colour and depth buffers, their sizes in VDIData.bufferSizes): one
 * self-describing byte stream of the bound VDI -- a 128-byte header (dimensions, entry count, the generating
 * camera's proj * view), a count per pixel, then the stored entries alone, depths and colours, in pixel order.
 * The same VDI always packs to the same bytes.  insitu_amd/vdi_io.py reads and writes the format without this
 * library.  The three calls work on the bound VDI on the view's own stream, so they are legal while a pipelined
 * frame is in flight, as insitu_view_render is.
 *
 * Bytes of the packed stream of the bound VDI in `format` (enum insitu_pack_format); 0 on error (no VDI bound,
 * bad format).  VolumeFromFileExample.kt:907-1030 (the sizes it sends ahead of the buffers). */
size_t insitu_view_pack_bytes(insitu_ctx* ctx, int format);
/* Pack the bound VDI into host_out (cap >= the size above) and block.  *bytes (may be NULL) = the stream's size,
 * also when cap is too small (then -1, and nothing is written to host_out).  VolumeFromFileExample.kt:907-1030
 * (the compaction and compression of the VDI before it is published). */
int insitu_view_pack(insitu_ctx* ctx, int format, void* host_out, size_t cap, size_t* bytes);
/* Bind the VDI of a packed stream (either format; W, H and S need not be the context's), as insitu_view_bind_host
 * does for the dense layout.  The header and `bytes` are checked on the host, the counts on the device before
 * anything is placed by them; a rejected stream returns -1.  The receiving end of
 * VolumeFromFileExample.kt:907-1030 (the remote viewer's upload of the message). */
int insitu_view_bind_packed(insitu_ctx* ctx, const void* data, size_t bytes);
/* Bind n (1..32) packed streams of one window and one generating camera as one merged VDI (an addition within ABI
 * 12: no existing call or structure changes).  streams[j] of bytes[j] bytes takes the place of slot j of
 * INSITU_VIEW_MERGED: the lists of a pixel are merged by start depth, the lowest stream first on a tie, entries
 * copied bit for bit, into S_m = max(1, the longest merged list) slots; more than 255 is rejected with -1.  Stream
 * j's list at a pixel is its first `count` entries, ending before the first one whose start depth is 0, so the call
 * binds what insitu_view_bind_host_set binds of the streams unpacked (vdi_io.unpack_vdi) and zero-padded to the
 * largest S -- without ever expanding them: the merge reads the streams' sections as they arrive (DESIGN.md section
 * 9.8).  W, H and pv_g (its 64 bytes) must agree across the set; S and the format may differ, a binary16 colour is
 * widened exactly.  Every stream is checked as insitu_view_bind_packed checks one, header and size on the host
 * before anything is allocated, counts on the device before any entry is read; a rejection returns -1 and names
 * the stream's index and the reason, and no VDI is left bound.  n = 1 is insitu_view_bind_packed of that stream.
 * Runs on the view's own stream: legal while a pipelined frame is in flight.  insitu_stats reports it through
 * view_slots, view_overlaps, view_entries, view_bytes, view_compact and ms_view_bind. */
int insitu_view_bind_packed_set(insitu_ctx* ctx, const void* const* streams, const size_t* bytes, int n);
/* Gather every rank's bound VDI into one merged VDI bound on rank 0 (an addition within ABI 12: no existing call or
 * structure changes) -- the whole scene without loss and without the host: what stands in for the MPI_Gather behind
 * DistributedVolumes.kt:903-904 and for a viewer that reads the per-rank SubVDI dumps of :848-849, with none of the
 * compositor's re-supersegmentation.  A collective over the context's ranks with rank 0 as the root: every rank has a
 * VDI bound (INSITU_VIEW_MERGED, say; any bind counts), and after a successful call the root has bound exactly what
 * insitu_view_bind_packed_set binds from the ranks' insitu_view_pack(format) streams in rank order, stream j = rank
 * j (a message about "stream j" is about rank j): merged per pixel by start depth, the lowest rank first on a tie,
 * entries copied bit for bit (INSITU_PACK_HALF: colours rounded to binary16 by the pack and widened exactly), S_m =
 * max(1, the longest merged list) slots, more than 255 rejected, in the layout INSITU_OPT_VIEW_COMPACT says on the
 * root; view_slots, view_overlaps, view_entries, view_bytes, view_compact and ms_view_bind describe it.  W, H and
 * pv_g (its 64 bytes) must agree across the ranks; S and the layout may differ.  Only fixed-size control data -- a
 * 128-byte header per rank, the verdict, the totals -- is read on the host: counts, depths and colours go from
 * device to device.
 * A peer's bound VDI is the same after the call as before it, whether the call succeeds or fails; only the root's
 * binding changes, and on any failure the root has nothing bound.  A rank that cannot take part (nothing bound, bad
 * `format`, a frame in flight, an allocation failure) still takes its turn, so that no rank is left waiting: the
 * root rejects the gather, every rank returns -1, and insitu_last_error names the rank and the reason on every rank.
 * The communicator is then ready for the next collective.  A failure of the counts' check on the device is the root's
 * alone: a peer has returned 0 once its sections were sent.
 * *wire_bytes (may be NULL): on the root the section bytes received from the peers, on a peer the section bytes it
 * sent, W*H + 8*E + (16 or 8)*E; 0 with one rank.  nranks = 1: insitu_view_bind_packed of the rank's own
 * insitu_view_pack(format) stream, whose entries take no host round trip either.  More than 32 ranks: -1 on every
 * rank, without communicating.
 * With nranks > 1 the call uses the context's communicator (on the view's stream), so -- unlike the other view calls
 * -- it is NOT legal while a pipelined frame is in flight: insitu_pipeline_flush first (a rank that has one refuses).
 * In a local group the calls are sequential, as insitu_gather's are, the peers first and the root last: a peer's call
 * packs, leaves its offer (header, section pointers, an event) and returns 0, also when it refuses; the root's call
 * validates the offers, pulls the sections device to device and binds, so a rejection is seen by the root alone.  A
 * root that calls before some peer has offered returns -1 and names that rank.  An offer holds the peer's staged
 * sections: a bind or a pack on the peer before the root's call withdraws it, and the root's call then fails. */
int insitu_view_gather_merged(insitu_ctx* ctx, int format, unsigned long long* wire_bytes);
int insitu_get_stats(insitu_ctx* ctx, insitu_stats* out);
/* Set a tuning option (enum insitu_option) for the following renders; -1 on an unknown option or
 * a value out of range.  Environment variables INSITU_<OPTION NAME> (INSITU_EXACT_SEARCH,
 * INSITU_SEARCH_DEPTH, ..., INSITU_VIEW_SKIP, INSITU_VIEW_COMPACT) seed the values when the context is created (tuning scripts). */
int insitu_set_option(insitu_ctx* ctx, int option, long long value);
/* Mean raymarch passes over rays that hit a brick, and the number of such rays, of the last
 * render over all local bricks (needs keep_passes; reads the pass buffer back). */
int insitu_pass_stats(insitu_ctx* ctx, double* mean_passes, long long* rays_hit);
void* insitu_stream(insitu_ctx* ctx);

/* ---- reference-shaped entry points (host ByteBuffers, reference layouts) ----
 * distributeVDIs(subVDIColor, subVDIDepth, sizePerProcess, commSize, colPointer, depthPointer,
 * mpiPointer), DistributedVolumes.kt:136-137 / DistributedVolumeRenderer.kt:112: all-to-all of
 * the host sub-VDI (VDI mode: sizePerProcess = H*W*S*4/commSize floats of colour per
 * destination, depth = half of that; plain mode: bytes of rgba8 per destination, same for
 * depth), received blocks written to recvColor/recvDepth (the native-owned
 * allToAllColorPointer/allToAllDepthPointer), then the composite of this rank's strip is run on
 * the GPU from them (what compositeVDIs/uploadForCompositing trigger). */
int insitu_distribute_vdis(insitu_ctx* ctx, const void* subVDIColor, const void* subVDIDepth,
                           long long sizePerProcess, int commSize, void* recvColor, void* recvDepth);

/* gatherCompositedVDIs(compositedVDIColor, compositedVDIDepth, compositedVDILen, root, myRank, commSize,
 * colPointer, depthPointer, mpiPointer), DistributedVolumes.kt:138-139 / :903-904 (composite_vdi
 * contexts): gathers the composited VDI strips on root 0; compositedVDILen = H*W*S_out*4/commSize
 * floats of colour per rank.  The root's gatherColor receives (S_out,H,W) rgba32f and gatherDepth
 * (2S_out,H,W) r32f (the native-owned gatherColorPointer/gatherDepthPointer); other ranks pass NULL. */
int insitu_gather_composited_vdi_set(insitu_ctx* ctx, long long compositedVDILen, int root, int myRank, int commSize,
                                     void* gatherColor, void* gatherDepth);

/* gatherCompositedVDIs(compositedVDIColor, root, subVDILen, myRank, commSize, ...)
 * (DistributedVolumeRenderer.kt:113, :602-603): gathers the composited rgba8 strips on root 0
 * (subVDILen = H*W*4/commSize bytes); the root's full image goes to gatherOut (what streamImage
 * receives, DistributedVolumeRenderer.kt:726).  Requires bricks_per_rank == 1 like the reference. */
int insitu_gather_composited_vdis(insitu_ctx* ctx, int root, long long subVDILen, int myRank, int commSize,
                                  void* gatherOut, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
