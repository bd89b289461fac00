/*
 * mtadgat.h -- C ABI of the MI355X-native MTAD-GAT per-window forward path.
 *
 * The reference (ML4ITS/mtad-gat-pytorch) is pure Python on PyTorch and has no
 * FFI of its own; the interface this library replaces is the Python call
 *
 *     predictions, recons = MTAD_GAT.forward(x)          reference mtad_gat.py:64-79
 *
 * and, stage by stage, the nn.Module.forward() methods it is made of
 * (reference modules.py, cited per entry point below).  The Python module
 * `mtad-gat-pytorch_amd/mtad_gat.py` mirrors the reference class on top of this
 * ABI through ctypes; any other host language binds the
 * same symbols.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a
 *     negative mtadgat_status; mtadgat_last_error() gives the message
 *     (thread-local).  Nothing throws across the boundary.
 *   - all tensors are float32, row-major contiguous, in the reference's own
 *     shapes -- with one exception: mtadgat_forward_xbf16 takes its input
 *     windows as bfloat16 (BASELINE config 2's "bf16 inference"); its outputs
 *     are float32 like everyone else's.  `*_dev` pointers are device (HBM)
 *     pointers owned by the caller, `*_host` pointers are host pointers.
 *   - every launch goes to the HIP stream the caller passes (a hipStream_t cast
 *     to void*; NULL = the null stream) and nothing synchronises the device.
 *   - the library keeps no per-call state besides the packed weights held by
 *     the handle.  A handle may be used from several streams one after
 *     another (weight packs one call derives on the device are waited for by
 *     later calls on other streams; the caller still orders its own buffers
 *     and weight uploads), but not from two host threads at once.
 *   - the model-path calls (mtadgat_forward, _forward_xbf16, _forward_series,
 *     _attention*, _series_losses, _score_attribution, _forward_train,
 *     _backward, _backward_input, _backward_data, the stage entries and
 *     _dropout_masks*) read and write nothing outside the buffers they are
 *     given: of an input or output exactly the elements of the stated shape,
 *     of a workspace or tape exactly the byte count passed with it (the count
 *     the matching *_bytes function reports is enough; nothing is rounded up on
 *     the caller's behalf), and what lies in front of or behind a buffer never
 *     influences a result.  Workspace and tape contents need not be
 *     initialised.  Their buffers need only the alignment stated per argument:
 *     workspace and tape 16 bytes (a too small or misaligned one is refused
 *     with MTADGAT_ERR_WORKSPACE before anything is launched), every other
 *     tensor of these calls the alignment of its element type -- 4 bytes for
 *     float32, 2 for the bfloat16 windows, 8 for int64 / float64 -- and their
 *     results do not depend on it bit for bit.  tests/test_gpu_guard_bands*.py
 *     hold these calls to this with guard-banded, exactly sized, misaligned
 *     buffers.
 *   - the same holds for the handle-free evaluation and preparation calls
 *     (mtadgat_eval_*, mtadgat_spot_state_bytes / _calibrate / _run / _copy,
 *     mtadgat_prep_fit / _transform / _inverse): of an (n, d) array with row
 *     stride ld exactly (n - 1) ld + d elements -- the last row ends behind
 *     its d-th element, and what lies between the rows is never read --, of
 *     scratch exactly the bytes the matching *_scratch function reports, or,
 *     for the calls that take no byte count (mtadgat_eval_moments,
 *     _epsilon_table, _point_adjust and the _columns forms), the minimum
 *     stated at their declarations; scratch and the SPOT state need the
 *     alignment stated there (8 or 16 bytes; short or misaligned scratch is
 *     refused with -5 before anything is launched), every other tensor the
 *     alignment of its element type.  Results do not depend on alignment or
 *     on what surrounds a buffer bit for bit, except the float64 sums of
 *     mtadgat_eval_moments / _epsilon_table and their _columns forms, which
 *     are combined with atomics and may differ in their last bits between
 *     any two calls (their counts are exact).
 *     tests/test_gpu_guard_bands_eval.py and _prep.py hold them to this.
 *     (The fit and stream calls -- mtadgat_fit_*, mtadgat_stream_*,
 *     mtadgat_prep_stream_* -- state the alignment of their scratch and state
 *     buffers at their declarations.)
 *   - gfx950 only.  There is no CPU implementation behind this ABI.
 */
#ifndef MTADGAT_H
#define MTADGAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTADGAT_ABI_VERSION 1
#define MTADGAT_MAX_LAYERS 8

typedef enum mtadgat_status {
    MTADGAT_OK = 0,
    MTADGAT_ERR_INVALID = -1,      /* bad argument / inconsistent shapes         */
    MTADGAT_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels cover       */
    MTADGAT_ERR_HIP = -3,          /* a HIP runtime call failed                  */
    MTADGAT_ERR_NOWEIGHTS = -4,    /* forward before mtadgat_load_weights        */
    MTADGAT_ERR_WORKSPACE = -5     /* workspace NULL; workspace or tape too small or misaligned */
} mtadgat_status;

/* Model hyper-parameters: the constructor arguments of reference
 * MTAD_GAT.__init__ (mtad_gat.py:37-54) after the defaulting that
 * modules.py:36-63 / :137-164 apply. */
typedef struct mtadgat_config {
    int32_t n_features;       /* F  (mtad_gat.py:39)                                   */
    int32_t window_size;      /* W  (mtad_gat.py:40)                                   */
    int32_t out_dim;          /* mtad_gat.py:41                                        */
    int32_t kernel_size;      /* odd; ConvLayer pads (k-1)/2, modules.py:14            */
    int32_t use_gatv2;        /* 1: GATv2 (modules.py:74-77), 0: GAT (modules.py:80-83)*/
    int32_t feat_embed;       /* rows of feature_gat.lin.weight  (doubled already for v2, modules.py:47-50) */
    int32_t time_embed;       /* rows of temporal_gat.lin.weight (modules.py:148-151)  */
    int32_t gru_n_layers;     /* modules.py:233                                        */
    int32_t gru_hid_dim;
    int32_t forecast_n_linear;/* number of nn.Linear in Forecasting_Model = n_layers+1 (modules.py:297-301) */
    int32_t forecast_hid_dim;
    int32_t recon_n_layers;   /* modules.py:253                                        */
    int32_t recon_hid_dim;
    float   alpha;            /* LeakyReLU negative slope (modules.py:62,163)          */
} mtadgat_config;

/* The reference's parameters (its state_dict, mtad_gat.py:56-62), as host
 * pointers to float32 arrays in the reference's own shapes. */
typedef struct mtadgat_params {
    const float* conv_weight;      /* conv.conv.weight   (F, F, k)                     */
    const float* conv_bias;        /* conv.conv.bias     (F)                           */
    const float* feat_lin_weight;  /* feature_gat.lin.weight  v2 (E_f, 2W)  v1 (E_f, W)*/
    const float* feat_lin_bias;    /* feature_gat.lin.bias    (E_f)                    */
    const float* feat_a;           /* feature_gat.a           v2 (E_f,1)   v1 (2E_f,1) */
    const float* feat_bias;        /* feature_gat.bias        (F, F)                   */
    const float* temp_lin_weight;  /* temporal_gat.lin.weight v2 (E_t, 2F)  v1 (E_t, F)*/
    const float* temp_lin_bias;    /* temporal_gat.lin.bias   (E_t)                    */
    const float* temp_a;           /* temporal_gat.a          v2 (E_t,1)   v1 (2E_t,1) */
    const float* temp_bias;        /* temporal_gat.bias       (W, W)                   */
    /* gru.gru.{weight_ih,weight_hh,bias_ih,bias_hh}_l<i>; gate order r|z|n            */
    const float* gru_w_ih[MTADGAT_MAX_LAYERS];   /* (3H, 3F) for l0, (3H, H) after     */
    const float* gru_w_hh[MTADGAT_MAX_LAYERS];   /* (3H, H)                            */
    const float* gru_b_ih[MTADGAT_MAX_LAYERS];   /* (3H)                               */
    const float* gru_b_hh[MTADGAT_MAX_LAYERS];   /* (3H)                               */
    /* forecasting_model.layers.<i>.{weight,bias}                                      */
    const float* fc_weight[MTADGAT_MAX_LAYERS];
    const float* fc_bias[MTADGAT_MAX_LAYERS];
    /* recon_model.decoder.rnn.*_l<i>                                                  */
    const float* rec_w_ih[MTADGAT_MAX_LAYERS];   /* (3Hr, H) for l0, (3Hr, Hr) after   */
    const float* rec_w_hh[MTADGAT_MAX_LAYERS];
    const float* rec_b_ih[MTADGAT_MAX_LAYERS];
    const float* rec_b_hh[MTADGAT_MAX_LAYERS];
    const float* rec_fc_weight;    /* recon_model.fc.weight (out, Hr)                  */
    const float* rec_fc_bias;      /* recon_model.fc.bias   (out)                      */
} mtadgat_params;

typedef struct mtadgat_handle_s* mtadgat_handle;

int         mtadgat_abi_version(void);
const char* mtadgat_last_error(void);

/* Replaces MTAD_GAT.__init__ (mtad_gat.py:37-62): validates the configuration. */
int mtadgat_create(const mtadgat_config* cfg, mtadgat_handle* out);
int mtadgat_destroy(mtadgat_handle h);

/* Replaces load_state_dict / the in-place parameter update seen by forward()
 * (training.py:127, :248; utils.py:189): re-packs the parameters into the
 * kernels' tile format on the host and uploads them on `stream`.  Call again
 * whenever a parameter changed. */
int mtadgat_load_weights(mtadgat_handle h, const mtadgat_params* params_host, void* stream);

/* The same for parameters that are already in device memory -- the training loop's optimizer.step() followed by a
 * forward (training.py:127 -> :110): `flat_dev` holds all parameters back to back in the field order of
 * mtadgat_params (the order of the flat gradient buffer, mtadgat_grad_offsets / mtadgat_grad_floats), and the tile
 * image is rebuilt from it by kernels on `stream`; nothing travels to the host and nothing synchronises (the column order of
 * the folded GATv2 projection follows the signs of the attention vectors `a`: derived on the device since round 5, the kernels
 * read the sign-group boundaries from the image).  Requires one
 * earlier mtadgat_load_weights on this device and precision mode 0 or 2 (the fp32 image; the split-operand packs of mode 2
 * are re-derived from it on the device); mode 1 returns MTADGAT_ERR_UNSUPPORTED (callers then use
 * mtadgat_load_weights).  The bf16 weight streams are not maintained: mtadgat_bf16_ready turns 0. */
int mtadgat_update_weights_device(mtadgat_handle h, const float* flat_dev, int64_t n_floats, void* stream);

/* Bit-exact 64-bit checksum of a list of device tensors of 32-bit elements (the model's parameters), written to
 * *out_dev on `stream`: one launch.  The Python module compares it between calls to notice in-place parameter edits
 * that autograd's version counters do not see (p.data.mul_(), nn.init.*_(p.data)). */
int mtadgat_params_fingerprint(const void* const* tensors_dev, const int64_t* n_elements, int n_tensors, uint64_t* out_dev, void* stream);

/* Host-only self check of the gather table behind mtadgat_update_weights_device (needs no GPU): packs `params_host`
 * with the host packer, derives the table, and returns the number of image positions the table would fill with a value
 * different from the host packer's (0 = consistent; negative = error).  *n_gathered: positions the table covers. */
int64_t mtadgat_selfcheck_gather_table(mtadgat_handle h, const mtadgat_params* params_host, int64_t* n_gathered);

/* Diagnostic: copies the packed weight image (mtadgat_packed_floats floats) to host memory after synchronising
 * `stream` -- the tests compare the device-side re-pack with the host packer through it. */
int64_t mtadgat_packed_floats(mtadgat_handle h);
/* (offset, length) pairs in floats of the image regions that are derived on the device from other regions of the image
 * (the split packs); returns their number (at most max_pairs are written).  out_pairs_host == NULL with max_pairs == 0 returns
 * the number only. */
int mtadgat_derived_regions(mtadgat_handle h, int64_t* out_pairs_host, int max_pairs);
int mtadgat_read_packed(mtadgat_handle h, float* dst_host, int64_t n_floats, void* stream);
/* Test hook (host only: needs neither a GPU nor loaded weights): the table of steps that derive the split packs from the fp32
 * packs of the image, over all groups in group order, then step order.  A record is 10 int64:
 *   [group, op, scale, src, dst, n, Qs, Qd, arg, ord]
 *   op     0 ZERO_SCALE, 1 ABSMAX, 2 SCALE_FROM_MAX, 3 SPLIT3, 4 SPLIT2H, 5 SPLIT2H_GATH, 6 SPLIT_X, 7 REORDER_XQ
 *   scale  offset (floats) of the group's scale slot [bits of max |W|, S, 1 / S, 0] (0: the step uses none)
 *   src, dst  offsets (floats) of the pack read and of the region written
 *   n      ABSMAX: floats of src; the others: outer count (tiles; SPLIT2H_GATH: tiles per side)
 *   Qs, Qd  chunks per tile of src / dst
 *   arg    SPLIT2H: words per chunk (gates); SPLIT_X: leading chunks on three bf16 pieces; SPLIT2H_GATH: embedding columns E
 *   ord    SPLIT2H_GATH: offset of the layer's column order [P8, PT, npos, 0] (ints)
 * Returns the number of steps; at most max_steps records are written (out_host == NULL with max_steps == 0 returns the number only).
 * mtadgat_split_n_infer: groups [0, n_infer) are what an inference call may read (mtadgat_read_packed derives those), the rest
 * belong to the training backward. */
int mtadgat_split_steps(mtadgat_handle h, int64_t* out_host, int max_steps);
int mtadgat_split_n_infer(mtadgat_handle h);
/* Test hook: derives every stale split group, the training backward's included, on `stream` -- what the kernels' callers do lazily,
 * group by group.  Needs loaded weights.  mtadgat_read_packed afterwards shows every pack current. */
int mtadgat_derive_split_packs(mtadgat_handle h, void* stream);
/* Test hook (host only: needs neither a GPU nor loaded weights): which kernels run one recurrence layer.  stack 0: the GRU stack,
 * 1: the reconstruction decoder; `layer` counts from the input; n: windows of the call (one piece of a forward(), or one training
 * forward); compute_units: of the device the call would run on (256 on MI355X).  The answer is the one the library's own dispatch
 * uses -- for a forward() that returns predictions and reconstructions, or a training forward -- under the handle's current
 * mtadgat_set_precision mode and "gru_kernel" option.  Writes 8 ints:
 *   out_host[0]  first kernel: 1 k_gru1 (window per workgroup), 2 k_gru16 (16-window groups), 3 k_gru_split (hidden-tile split),
 *           4 k_gru_split on split operands, 5 k_gru_cm (chunk-major), 6 k_gru (tile-major)
 *   out_host[1]  kernel launched behind it as the device-side range-guard fallback (same codes), 0 none
 *   out_host[2]  operand build of the k_gru_split / k_gru named in out_host[0] / out_host[1]: 0 fp32, 1 bf16, 2 / 3 split-bf16 (hidden sizes
 *           above / up to 128); 0 when neither is named
 *   out_host[3]  k_gru takes two 32-window groups per wave
 *   out_host[4]  the input products of all steps are hoisted into a launch in front
 *   out_host[5]  the layer's split packs are needed (derived on first use after an upload)
 *   out_host[6]  the per-step Linear of the decoder rides inside the recurrence
 *   out_host[7]  the stack takes the small-batch kernels (what the heads and the training forward ask; equals out_host[0] in {1, 2} for layer 0)
 * Returns 0, or MTADGAT_ERR_INVALID. */
int mtadgat_gru_route(mtadgat_handle h, int stack, int layer, int64_t n, int training, int compute_units, int* out_host);
/* Test hook (host only: needs neither a GPU nor loaded weights): which kernels run the front end -- window convolution, temporal
 * and feature attention layer -- of one call on n windows (one piece of a forward()).  The answer is the one the library's own
 * dispatch uses under the handle's current mtadgat_set_precision mode and "conv_kernel" / "gat_kernel" / "conv_fused" /
 * "conv_shared" / "rowgemm_kernel" options.
 *   kind    0 a whole inference forward (h_cat only, output range recorded; a model with an un-fused layer gets kind 1),
 *           1 the un-fused inference forward and mtadgat_gat (xc, xc^T, h_cat), 2 the training forward, 3 attention maps (fp32
 *           arithmetic whatever the mode), 4 mtadgat_conv (y only, no layers)
 *   source  0 float32 windows, 1 bfloat16 windows, 2 a series with stride 1 and no `starts`, 3 any other series
 *   facts   bit 0: the node rows the fused layers read are 16-byte aligned; bit 1: their row stride is a multiple of 4 floats and
 *           at least the node columns rounded up to 4; bit 2: h_cat is 16-byte aligned (all set in the library's own calls)
 * Writes 14 ints:
 *   out_host[0]  convolution: 0 none (inside the temporal layer's k_gath), 1 k_conv_win on fp16 pieces, 2 shared rows of a series
 *           (three launch_conv calls and the row placement), 3 launch_conv
 *   out_host[1]  operands of that launch_conv: 0 fp32, 1 the bf16 pack, 2 three bf16 pieces (rows too long for LDS staging)
 *   out_host[2]  the convolution's split packs are needed (derived on first use after an upload)
 *   out_host[3]  the convolution's output range is recorded for the kernels behind it
 *   out_host[4 .. 9) the temporal layer, out_host[9 .. 14) the feature layer:
 *     [0]  0 none, 1 fused k_gat alone, 2 k_gath with k_gat behind it as the device-side fallback, 3 row GEMM projection +
 *          k_gat_wide, 4 row GEMM projection + k_attend
 *     [1]  operands of the projection: 0 fp32, 1 bf16, 2 three bf16 pieces
 *     [2]  k_gat is handed the two-fp16-piece pack beside its bf16 pieces (never for a GATv2 layer without k_gath: its fp16
 *          pack is in k_gath's column order)
 *     [3]  the un-fused projection is the split row GEMM
 *     [4]  the layer's split packs are needed
 * Returns 0, or MTADGAT_ERR_INVALID. */
int mtadgat_front_route(mtadgat_handle h, int kind, int source, int64_t n, int facts, int* out_host);
/* Test hook (host only: needs neither a GPU nor loaded weights): how a forward call of `batch` windows is cut up and where each part
 * lives in the caller's workspace.  The answer is the one the library's own forward uses under the handle's current
 * mtadgat_set_chunk_windows size, mtadgat_set_precision mode and "lanes" option.  Writes 5 + 3 * n_pieces values:
 *   out_host[0]  n_pieces: pieces of the call, run in this order
 *   out_host[1]  1 when the call is small enough to run its independent stages side by side on the handle's second stream
 *   out_host[2]  floats of the workspace part of lane 0 (the caller's stream), which begins at the workspace's start
 *   out_host[3]  floats of the part of lane 1 (the handle's second stream), which begins out_host[2] floats in; 0 when no piece runs there
 *   out_host[4]  floats of the whole workspace: mtadgat_workspace_bytes / 4
 *   out_host[5 + 3 i .. 8 + 3 i)  piece i: its first window, its window count, its lane
 * Returns the count of values written, or MTADGAT_ERR_INVALID (a NULL argument, batch < 1, max_n too small: nothing is written). */
int mtadgat_forward_plan(mtadgat_handle h, int64_t batch, int64_t* out_host, int max_n);
/* Test hook (host only: needs neither a GPU nor loaded weights): which kernels run the recurrence layers and the attention layers of
 * a training step (mtadgat_forward_train + mtadgat_backward) of n windows.  The answer is the one the library's own dispatch uses
 * under the handle's current mtadgat_set_precision mode and "gru_kernel" option; the backward's recurrence kernel is derived from
 * the forward's, whose tape it reads.  Writes 3 * (gru_n_layers + recon_n_layers) + 5 ints:
 *   per layer of the GRU stack, then per layer of the decoder, counted from the input:
 *     [0]  first kernel of the training forward (the codes of mtadgat_gru_route's out_host[0])
 *     [1]  kernel of the backward: 0 k_gru1_bwd (partner of k_gru1), 1 k_gru16_bwd (partner of k_gru16), 2 k_gru_bwd (partner of
 *          k_gru_split on either operand build)
 *     [2]  k_gru_bwd multiplies on three bf16 pieces per operand (its split pack is derived on first use after an upload)
 *   then 1 when the decoder's per-step Linear runs inside the top decoder layer's recurrence in this call (its partial sums fit the
 *   hidden-tile-split kernel's LDS and the decoder is not on the small-batch kernels), 0 when it is a row GEMM over the kept states
 *   then for the feature and for the temporal attention layer:
 *     [0]  the backward goes through the generic wide-layer kernels (the layer is not fused)
 *     [1]  the score backward is GAT (v1)'s (use_gatv2 == 0)
 * Returns the count of values written, or MTADGAT_ERR_INVALID (a NULL argument, n < 1, max_n too small: nothing is written),
 * MTADGAT_ERR_UNSUPPORTED (the configuration has no HIP backward). */
int mtadgat_train_route(mtadgat_handle h, int64_t n, int* out_host, int max_n);
/* Test hook (host only: needs neither a GPU nor loaded weights): how the weight-gradient GEMMs (d W = A^T B over the rows of the
 * call, k_wgrad_lds + one batched reduction) of a backward of n windows -- one chunk of the training step -- are laid out.  The slab
 * plan is the one the library's own dispatch launches under the handle's current mtadgat_set_precision mode and "wgrad_kernel"
 * option.  Sites, in this order: the convolution; with GATv2 the projection of the feature layer, then of the temporal layer (GAT v1
 * has none: its parameter gradients come from column sums); W_ih then W_hh of every GRU layer, then of every decoder layer, counted
 * from the input; the decoder's per-step Linear; every forecasting Linear from the input.  Ten values per site:
 *   [0] R     rows: n * window for all but the feature projection (n * n_features) and the forecasting Linears (n)
 *   [1] M  [2] N      rows and columns of d W (the bias gradient rides as column N: an all-ones column of B)
 *   [3] Mp [4] Np     the partial blocks' padded sizes
 *   [5] nslab         row slabs (gridDim.y; a multiple of 8 enables the kernel's XCD-aware block map)
 *   [6] rows_per_slab a multiple of 16; slabs that start at or beyond R are empty and leave zero partials
 *   [7] bmode         1: B is the im2col view of the input windows (the convolution)
 *   [8] bshift        1: B is read one step earlier, masked at the first step of a window (W_hh)
 *   [9] x3            products from three bf16 pieces per operand, 0: the fp32 MFMA
 * (Whether a site stages float4 or dword loads depends on the alignment of the call's buffers and is not reported.)
 * Returns the count of values written, or MTADGAT_ERR_INVALID (a NULL argument, n < 1, max_n too small: nothing is written),
 * MTADGAT_ERR_UNSUPPORTED (the configuration has no HIP backward). */
int mtadgat_wgrad_plan(mtadgat_handle h, int64_t n, int64_t* out_host, int max_n);
/* Test hook (host only): does a row GEMM over `rows` rows take split-bf16 operands (k_rowgemm_x3) under the handle's precision mode
 * and "rowgemm_kernel" option?  has_pack: a split pack was planned for its weights; backward: a site of mtadgat_backward (there
 * "rowgemm_kernel" = 2 forces the split pack in every mode, in the forward only in the "fp32" mode).  Returns 1 / 0, negative: error. */
int mtadgat_rowgemm_split(mtadgat_handle h, int has_pack, int64_t rows, int backward);

/* Arithmetic of the inference entry points (forward / forward_series / stage calls):
 *   0 (default of a new handle)  fp32 operands on the exact fp32 MFMA: <= 1e-5 of the reference's float32 forward
 *   2            fp32 results, the products of the large-batch kernels (k_gru above 16 384 windows, the attention
 *                projection above 4 096) formed from split 16-bit operands: every fp32 operand is the exact sum of three
 *                bf16 pieces (six MFMA terms with fp32 accumulation per product) or, where its range is bounded by
 *                construction -- recurrent state, attention outputs, weights scaled by a per-layer power of two --, of
 *                two fp16 pieces (three terms): within ~2e-7 of mode 0, same 1e-5 gate, 2.7-5x less matrix-pipe time
 *                on the pipe that runs beside the VALU (the Python module's default).
 *                The split weight packs are derived on the device by the first launch that reads them after a load
 *                (round 6; rounds 2-5: at every load); switching needs no reload.
 *   1            bf16 MFMA operands (weights packed to bf16 once per load_weights, activations rounded on the
 *                way into the matrix unit), fp32 accumulation, fp32 recurrent state / gates / softmax:
 *                <= 2e-2 of the fp32 reference on outputs of scale ~1 (BASELINE configs "bf16 inference").
 *                From 4 096 windows per chunk the convolution and the two attention layers run on mode 2's two-fp16-piece
 *                kernels instead (faster than their bf16 builds and closer to fp32); the recurrences and heads stay bf16.
 * The training entry points (mtadgat_forward_train / mtadgat_backward) compute in fp32 -- modes 0 and 2 -- and REFUSE mode 1
 * (MTADGAT_ERR_UNSUPPORTED): the bf16-operand recurrences of rounds 2-5 were slower than the fp32 step at every batch size and
 * were removed in round 6. */
int mtadgat_set_precision(mtadgat_handle h, int mode);
/* The bf16 weight streams are packed by mtadgat_load_weights only while mode 1 is selected (select first, or load
 * again after switching); 1 when they are present. */
int mtadgat_bf16_ready(mtadgat_handle h);

/* Testing / measurement hook (not needed for normal use).  "gru_kernel": which kernel runs the large-batch recurrences
 * (GRULayer.forward modules.py:235-238, the decoder modules.py:276-283) in precision mode 2:
 *   0 automatic (default), 1 the tile-major kernel at every batch size, 2 the chunk-major kernel wherever it applies,
 *   3 the hidden-tile-split kernel on split operands wherever it applies.
 * "gat_kernel": which kernel runs the fused attention layers (modules.py:65-95, :166-193) in precision mode 2:
 *   0 automatic (default: from 4096 windows per chunk the fp16-piece build k_gath of the row-split kernel when the convolution's
 *   outputs are below 2^15, else k_gat), 1 k_gat at every batch size, 3 k_gath at every batch size (2 was round 4's
 *   column-sliced kernel, removed: it lost to k_gath on every shipped shape).
 * "conv_kernel": the convolution of the fused front end (modules.py:18-22) in precision mode 2: 0 automatic (the
 *   window-per-workgroup kernel on fp16 pieces from 4096 windows per chunk), 1 k_conv_lds (fp32 MFMA), 2 k_conv_win at any size.
 * "conv_fused": 0 automatic -- in precision mode 2, wherever k_conv_win and k_gath both apply (from 4096 windows per chunk), the
 *   workgroup that runs the temporal attention layer on a window computes that window's convolution itself (mtad_gat.py:67-70 is
 *   one dataflow): no convolution launch, h_cat[:, :F] written once and not read back by that layer; the fp16 range guard is then
 *   per window.  1: always two launches.
 * "conv_shared": stride-1 series scoring in precision mode 2: 0 automatic (k_conv_win reads each window out of the series where it
 *   applies, the shared-row convolution of k_conv_lds otherwise), 1 the shared-row convolution wherever it applies.
 * ("series_band", the shared temporal pair scores of rounds 4-5, is gone: the option is refused.)
 * "rowgemm_kernel": the data-gradient products d X = d Y W of mtadgat_backward: 0 automatic (three bf16 pieces per operand from
 *   4096 rows in precision mode 2), 1 fp32 MFMA, 2 the split-bf16 build always.
 * "gemm_lds" (process-wide, not per handle): the split-bf16 row GEMMs and the wide models' convolution on launches of >= 131 072
 *   rows (Linear / Conv1d layers: modules.py:18-22, :76-81, :176-181; the data gradients of training.py:126): 0 automatic -- a
 *   workgroup of four waves owns 256 rows and shares each chunk's weight words through LDS; 1 the one-wave kernels everywhere
 *   (results are bit-identical either way).
 * "lanes": 0 automatic: mtadgat_forward / _forward_series walk calls of 8 193 .. 16 384 (two halves; 8 192 + the rest when the rest
 *   is at most 1 536 windows) and of more than 32 768 windows per chunk (whole 32 768-window pieces, then the rest) in
 *   pieces that alternate between `stream` and a second stream owned by the handle (each with its own half of the workspace;
 *   `stream` waits for the second lane before the call's work on it counts as complete, so the caller's ordering rules do not
 *   change); results = those of the call on each piece.  Models on the un-fused (wide) attention path alternate the CHUNKS of a call
 *   between the two streams (first piece: half a chunk).  1: everything on `stream`.
 * "gath_dbg": measurement hooks of k_gath (knock-outs: results invalid; sensitivity probes: results unchanged), csrc/mtadgat_kernels.h.
 * "wgrad_kernel": the weight-gradient GEMMs of mtadgat_backward (training.py:126): 0 automatic (three bf16 pieces per operand on
 *   the 16-bit matrix pipe in precision mode 2), 1 fp32 MFMA, 2 the split-bf16 build in every mode. */
int mtadgat_set_option(mtadgat_handle h, const char* name, int value);
/* Diagnostics for bench.py: the largest convolution output of the last forward() that used workspace `ws` (its last
 * chunk; synchronises `stream`).  Below 2^15 the large-batch kernels used two fp16 pieces per operand, otherwise three
 * bf16 pieces for the convolution's channels (device-side range guard). */
int mtadgat_last_conv_max(mtadgat_handle h, const void* ws_dev, int64_t batch, float* out_host, void* stream);

/* Bytes of device scratch forward() needs for a batch of `batch` windows
 * (intermediates of at most mtadgat_chunk_windows() windows are live at once). */
size_t  mtadgat_workspace_bytes(mtadgat_handle h, int64_t batch);
int64_t mtadgat_chunk_windows(mtadgat_handle h);
int     mtadgat_set_chunk_windows(mtadgat_handle h, int64_t windows);

/* Non-finite input (every forward entry point below, mtadgat_series_losses, mtadgat_stream_push and mtadgat_forward_train).
 * A sample is non-finite if it is NaN, +inf or -inf -- a "gap" of mtadgat_prep_*.
 *   - A window that holds a non-finite sample answers NaN in preds, in EVERY element of recons and in recons_last, in every
 *     precision mode, for float32 and bfloat16 input: what the reference's float32 algebra gives (the convolution spreads the sample
 *     over all channels, each attention layer's softmax makes the whole layer output NaN, the GRU carries it to h_end).
 *   - No other window of the call changes, beyond what a change of kernel allows: a launch-wide range guard may send the launch to
 *     its fallback kernel (results within the tolerance of the precision mode, not bit-equal).
 *   - A series: the affected windows are exactly those whose rows [s_w, s_w + W) contain the sample.
 *   - A stream (mtadgat_stream_push): the affected rows are those of that stream only -- the row itself and the next W rows score
 *     NaN and are not flagged; the row after that scores again.
 *   - mtadgat_forward_train's preds / recons follow the same rule, so the loss a caller forms from them is NaN and seen.
 *   - hend_dev, gradients (mtadgat_backward*), attention maps and attributions of non-finite input are unspecified.
 * The kernels upstream are not NaN-transparent (ReLU as fmaxf, clamped gate functions): the decision is taken per window at the
 * input and written over the outputs behind the heads (k_poison_nonfinite). */

/* Replaces MTAD_GAT.forward (mtad_gat.py:64-79), eval mode.
 *   x_dev      (batch, W, F)          in, not modified
 *   preds_dev  (batch, out_dim)       out   (may be NULL: skip both heads if recons_dev is NULL too)
 *   recons_dev (batch, W, out_dim)    out
 *   hend_dev   (batch, gru_hid_dim)   out, optional (NULL to skip): h_end of mtad_gat.py:74 */
int mtadgat_forward(mtadgat_handle h, const float* x_dev, int64_t batch,
                    float* preds_dev, float* recons_dev, float* hend_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* mtadgat_forward with the input given as bfloat16 (batch, W, F): the convolution reads it directly, no fp32 copy
 * of x is made (BASELINE "bf16 inference"; outputs stay float32).  MTADGAT_ERR_UNSUPPORTED for n_features beyond
 * the LDS-staged convolution. */
int mtadgat_forward_xbf16(mtadgat_handle h, const void* x_bf16_dev, int64_t batch, float* preds_dev, float* recons_dev,
                          float* hend_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Same as mtadgat_forward, with the windows gathered on the GPU from a device-resident series instead of
 * materialised by the caller: window w = series rows [s_w, s_w + W), s_w = starts_dev[w] when starts_dev is
 * not NULL, else start0 + w * stride.  Replaces SlidingWindowDataset.__getitem__ + default collate feeding
 * forward() (utils.py:107-120, prediction.py:43-44, 51-55): consecutive windows share W-1 rows, so the input
 * read from HBM shrinks ~W-fold.
 *   series_dev (n_rows, F) float32;  starts_dev (batch) int64 or NULL;  every window must lie inside the series.
 *   recons_last_dev (batch, out_dim), optional: recons[:, -1, :] only (what Predictor.get_score keeps,
 *   prediction.py:63); recons_dev may then be NULL and the full (batch, W, out_dim) tensor is never written. */
int mtadgat_forward_series(mtadgat_handle h, const float* series_dev, int64_t n_rows,
                           const int64_t* starts_dev, int64_t start0, int64_t stride, int64_t batch,
                           float* preds_dev, float* recons_dev, float* recons_last_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- stage entry points (the reference's sub-module forward() calls) ---------
 * Same workspace / stream contract; each is what forward() runs for that stage. */

/* ConvLayer.forward, modules.py:18-22: x (batch,W,F) -> y (batch,W,F). */
int mtadgat_conv(mtadgat_handle h, const float* x_dev, int64_t batch, float* y_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* FeatureAttentionLayer.forward (modules.py:65-95) when which == 0,
 * TemporalAttentionLayer.forward (modules.py:166-193) when which == 1:
 * xc (batch,W,F) -> h (batch,W,F). */
int mtadgat_gat(mtadgat_handle h, int which, const float* xc_dev, int64_t batch, float* h_dev,
                void* workspace_dev, size_t workspace_bytes, void* stream);

/* GRULayer.forward, modules.py:235-238: h_cat (batch,W,3F) -> h_end (batch,H)
 * (the h[-1] the reference keeps; its out[-1] is discarded by mtad_gat.py:73). */
int mtadgat_gru(mtadgat_handle h, const float* hcat_dev, int64_t batch, float* hend_dev,
                void* workspace_dev, size_t workspace_bytes, void* stream);

/* Forecasting_Model.forward (modules.py:307-311) and ReconstructionModel.forward
 * (modules.py:276-283): h_end (batch,H) -> preds (batch,out), recons (batch,W,out). */
int mtadgat_heads(mtadgat_handle h, const float* hend_dev, int64_t batch,
                  float* preds_dev, float* recons_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- attention maps ----------------------------------------------------------------------------
 * The post-softmax matrices of the two graph-attention layers -- `attention` of FeatureAttentionLayer.forward
 * (modules.py:85-89, nodes = features) and of TemporalAttentionLayer.forward (modules.py:184-188, nodes = time steps) --
 * in eval mode (no dropout): row i = softmax over the keys j.  Only the convolution and the attention layers run.
 *   att_feat_dev (batch, F, F) and att_temp_dev (batch, W, W), float32, out.  Either may be NULL: that layer does not run.
 * Arithmetic: the fp32 builds the training forward keeps its softmax rows with, in EVERY precision mode -- the maps do not
 * depend on mtadgat_set_precision, and a handle in mode 1 is served like one in mode 0.  The call leaves no state behind:
 * a later mtadgat_forward on the handle returns what it returned before, bit for bit.
 * The batch is walked in chunks of mtadgat_chunk_windows() windows.  batch < 1 returns MTADGAT_ERR_INVALID.
 * Workspace: mtadgat_attention_workspace_bytes(h, batch, 0), 16-byte aligned. */
size_t mtadgat_attention_workspace_bytes(mtadgat_handle h, int64_t batch, int reduce);
int mtadgat_attention(mtadgat_handle h, const float* x_dev, int64_t batch, float* att_feat_dev, float* att_temp_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same for the windows of mtadgat_forward_series (series_dev (n_rows, F), starts_dev or start0 + w * stride): the windows
 * are gathered from the series, not materialised. */
int mtadgat_attention_series(mtadgat_handle h, const float* series_dev, int64_t n_rows, const int64_t* starts_dev, int64_t start0,
                             int64_t stride, int64_t batch, float* att_feat_dev, float* att_temp_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);
/* Mean over the call's windows only: mean_feat_dev (F, F), mean_temp_dev (W, W).  The per-window maps pass through the
 * workspace a chunk at a time (chunks of at most mtadgat_chunk_windows() windows and 2^26 map floats), so the workspace --
 * mtadgat_attention_workspace_bytes(h, batch, 1) -- is bounded by one chunk.  The reduction is a fixed-order compensated fp32
 * sum without atomics (k_att_mean_part / k_att_mean_final): identical calls give identical bits for a given chunk size. */
int mtadgat_attention_mean(mtadgat_handle h, const float* x_dev, int64_t batch, float* mean_feat_dev, float* mean_temp_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);
int mtadgat_attention_series_mean(mtadgat_handle h, const float* series_dev, int64_t n_rows, const int64_t* starts_dev,
                                  int64_t start0, int64_t stride, int64_t batch, float* mean_feat_dev, float* mean_temp_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- forecast and reconstruction errors of a series ------------------------------------------------
 * What Trainer.evaluate (training.py:188-228) computes from model(x), for the windows of mtadgat_forward_series, without the
 * (batch, W, out_dim) reconstructions ever existing in full: the windows are cut into consecutive chunks of
 * L = mtadgat_series_losses_chunk(h) windows -- min(mtadgat_chunk_windows(h), max(1, 2^26 / (W out_dim))) -- and for each chunk
 * the forward writes preds and recons into the workspace and mtadgat_eval_window_sse (below, with its arithmetic and its
 * definitions) reduces them against the series, accumulate = (chunk > 0):
 *   window_sse_dev (batch, 2) float64 and dim_sse_dev (2, out_dim) float64 (may be NULL), both out.
 *   dims_dev (out_dim) int32: the series columns the outputs are compared with (NULL: 0 .. out_dim - 1, which needs out_dim <= F).
 * Chunk c's preds and recons are bit for bit what mtadgat_forward_series returns for that chunk's windows called on its own, in
 * the handle's current precision mode.  The call leaves no state behind: a later mtadgat_forward on the handle returns what it
 * returned before, bit for bit.  Identical calls give identical bits for a given chunk size.
 * batch >= 1; every window's target row must exist: with starts_dev NULL, start0 + (batch - 1) stride + W <= n_rows - 1 is
 * checked on the host.  Workspace: mtadgat_series_losses_workspace_bytes(h, batch), 16-byte aligned -- the forward workspace
 * of min(batch, L) windows, one chunk of preds and recons, and the reduction's scratch: it does not grow with batch beyond L. */
int64_t mtadgat_series_losses_chunk(mtadgat_handle h);
size_t mtadgat_series_losses_workspace_bytes(mtadgat_handle h, int64_t batch);
int mtadgat_series_losses(mtadgat_handle h, const float* series_dev, int64_t n_rows, const int64_t* starts_dev, int64_t start0,
                          int64_t stride, int64_t batch, const int32_t* dims_dev, double* window_sse_dev, double* dim_sse_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
/* mtadgat_series_losses_masked: the same chunk loop with the reduction over observed samples only (mtadgat_fit_masked_sse below,
 * with its age_dev (n_rows, F) int32 of row stride ld_age, and max_age): window_dev (batch, 4) float64 = (S_f, S_r, N_f, N_r) per
 * window, dim_dev (4, out_dim) float64 the same per output dimension (may be NULL).  Everything else as mtadgat_series_losses: the
 * chunk size, a chunk's outputs bit for bit those of mtadgat_forward_series, no state left behind, a workspace --
 * mtadgat_series_losses_masked_workspace_bytes(h, batch) -- bounded by one chunk. */
size_t mtadgat_series_losses_masked_workspace_bytes(mtadgat_handle h, int64_t batch);
int mtadgat_series_losses_masked(mtadgat_handle h, const float* series_dev, int64_t n_rows, const int64_t* starts_dev, int64_t start0,
                                 int64_t stride, int64_t batch, const int32_t* dims_dev, const int32_t* age_dev, int64_t ld_age,
                                 int32_t max_age, double* window_dev, double* dim_dev, void* workspace_dev, size_t workspace_bytes,
                                 void* stream);

/* ---- training step --------------------------------------------------------------------------------
 * Replaces what autograd does for the reference around MTAD_GAT.forward in Trainer.fit
 * (training.py:106-127: preds, recons = model(x); loss.backward()): a forward that keeps the
 * activations the backward needs in a caller-owned "tape" and applies dropout inside the kernels
 * (attention matrices modules.py:90 / :189, forecasting layers modules.py:310), and the backward
 * that turns d loss / d preds, d loss / d recons into the gradients of all parameters.
 *
 * Dropout is counter based: the mask of window `window0 + w` depends only on (seed, site, that global
 * window index, element), so chunking, sharding or recomputing a batch reproduces the same masks.
 * dropout_p = 0 gives the deterministic (eval-mode) function, e.g. for gradients in eval().
 *
 * Gradients are ACCUMULATED (+=) into `grads_dev`, a flat float32 buffer of mtadgat_grad_floats()
 * entries holding the reference's parameters' gradients in their own shapes, in the field order of
 * mtadgat_params (offsets: mtadgat_grad_offsets); zero it before the first chunk of a step.
 * Every configuration the forward accepts has a HIP backward (mtadgat_backward_supported: GATv2 and GAT (v1), any number of stacked
 * GRU / decoder layers; attention layers with more than 128 nodes or features -- up to 2048 -- run the kernels of
 * csrc/mtadgat_bwdw.hip with every matrix through memory; the GATv2 score backward of ALL layers is that file's one-pass k_bw_pair
 * behind a projection row GEMM since round 6).  `batch` windows are processed as one
 * chunk: tape and workspace grow linearly with it (~0.85 + 0.85 MB per window at W=100, F=55). */
int     mtadgat_backward_supported(mtadgat_handle h);
size_t  mtadgat_tape_bytes(mtadgat_handle h, int64_t batch);
size_t  mtadgat_backward_workspace_bytes(mtadgat_handle h, int64_t batch);
int64_t mtadgat_grad_floats(mtadgat_handle h);
/* offsets (floats) of conv w,b | feature lin w,b,a,bias | temporal lin w,b,a,bias | gru w_ih,w_hh,b_ih,b_hh |
 * fc (w,b) x forecast_n_linear | decoder w_ih,w_hh,b_ih,b_hh | recon fc w,b; returns the count */
int     mtadgat_grad_offsets(mtadgat_handle h, int64_t* offsets_host, int max_n);
int mtadgat_forward_train(mtadgat_handle h, const float* x_dev, int64_t batch, int64_t window0, float dropout_p,
                          uint64_t seed, float* preds_dev, float* recons_dev, void* tape_dev, size_t tape_bytes,
                          void* stream);
int mtadgat_backward(mtadgat_handle h, const float* x_dev, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                     const float* d_preds_dev, const float* d_recons_dev, const void* tape_dev, size_t tape_bytes,
                     float* grads_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Gradient with respect to the input windows (the reference's autograd provides it when x.requires_grad: mtad_gat.py:64-79 under
 * training.py:126; none of its callers asks).  Call right after mtadgat_backward of the same chunk, on the same stream, with the
 * same workspace: the convolution's pre-activation gradients are still in it.  dx_dev: (batch, W, F) float32, overwritten.
 * Covers every window shape the training step takes: windows of at most 64 KB (W F floats) keep one window per workgroup in LDS
 * (k_conv_dx); larger ones run d x as a forward-style convolution of the pre-activation gradients with the flipped, transposed
 * kernel w'[i][o][j] = w[o][i][k-1-j] (no bias, no ReLU) on the fp32 MFMA (k_conv over a pack of w' kept for such models). */
int mtadgat_backward_input(mtadgat_handle h, int64_t batch, const void* workspace_dev, size_t workspace_bytes, float* dx_dev, void* stream);
/* The data-only backward: mtadgat_backward's data path for one chunk -- every data gradient through the heads, recurrences,
 * attention layers and convolution, then the input gradient into dx_dev (batch, W, F), overwritten -- without a single
 * weight-gradient GEMM, column sum or reduction, and without a gradient buffer.  dx is bit-identical to mtadgat_backward followed
 * by mtadgat_backward_input on the same chunk.  Arguments as mtadgat_backward's (x_dev is not read and may be NULL); workspace:
 * mtadgat_backward_workspace_bytes. */
int mtadgat_backward_data(mtadgat_handle h, const float* x_dev, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                          const float* d_preds_dev, const float* d_recons_dev, const void* tape_dev, size_t tape_bytes, float* dx_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- score attribution -------------------------------------------------------------------------------------------------
 * Which input rows and channels pushed an anomaly score up.  For a series (N, F), window W and score index i with
 * 0 <= i < N - W (the index into the per-timestamp score of Predictor.get_score, prediction.py:65-91; the scored row is
 * series[i + W]):
 *   slice S = series[i : i+W+1] (W+1 rows); window A = S[0:W], window B = S[1:W+1], target y = S[W, dims]
 *   a_i(S) = sum_d w_d * ( |yhat_A[d] - y[d]| + gamma * |r_B[W-1, d] - y[d]| ),  yhat_A = preds of A, r_B = recons of B
 * w_d = 1 / n_dims, or with scaled scores 1 / (n_dims (1 + IQR_d)), IQR_d held constant (the caller computes it).  The model is the
 * eval-mode function (no dropout); the arithmetic is fp32.
 *   steps == 0 (gradient):            out = d a_i / d S                                   (W+1, F), sign(0) = 0
 *   steps == m > 0 (Integrated Grad.): out = (S - b) * (1/m) sum_{k<m} d a_i / d S at b + alpha_k (S - b), alpha_k = (k + 1/2) / m
 * Baseline b: baseline_kind 0 zeros (baseline_dev unused), 1 one (F) row for every step of the slice, 2 a (W+1, F) slice.
 *   series_dev (n_rows, F) float32; idx_dev (count) int64 score indices, each in [0, n_rows - W) -- not checked on the device;
 *   dims_dev (n_dims) int32 series column of each output dimension (n_dims == out_dim), each in [0, F); dim_w_dev (n_dims) float32 w_d;
 *   out_dev (count, W+1, F) float32, overwritten.
 * The 2 * count * max(steps, 1) windows are evaluated in chunks of at most mtadgat_chunk_windows() windows and ~4 GiB of scratch
 * (training forward without dropout, then mtadgat_backward_data); the sum over the steps is added in step order by one thread per
 * output element: no atomics, identical calls give identical bits.  The precision mode is set for the call -- 0 stays 0, 1 and 2
 * run as 2 (fp32-class) -- and restored afterwards.  MTADGAT_ERR_UNSUPPORTED when mtadgat_backward_supported is 0.
 * Workspace: mtadgat_score_attribution_workspace_bytes(h, count, steps), 16-byte aligned. */
size_t mtadgat_score_attribution_workspace_bytes(mtadgat_handle h, int64_t count, int steps);
int mtadgat_score_attribution(mtadgat_handle h, const float* series_dev, int64_t n_rows, const int64_t* idx_dev, int64_t count,
                              const int32_t* dims_dev, int n_dims, const float* dim_w_dev, float gamma, int steps,
                              const float* baseline_dev, int baseline_kind, float* out_dev, void* workspace_dev, size_t workspace_bytes,
                              void* stream);
/* Diagnostics for the tests: the keep-masks (1 / 0) the kernels apply -- mask_feat (batch, F, F), mask_temp
 * (batch, W, W), mask_fc (forecast_n_linear - 1, batch, forecast_hid_dim), any may be NULL -- and the offsets
 * (floats) of the tape / backward-workspace regions (order: see mtadgat_capi.cpp). */
int mtadgat_dropout_masks(mtadgat_handle h, int64_t batch, int64_t window0, float dropout_p, uint64_t seed,
                          float* mask_feat_dev, float* mask_temp_dev, float* mask_fc_dev, void* stream);
/* ... and of nn.GRU's dropout between stacked layers (reference modules.py:233, :253; training only): mask_gru
 * (gru_n_layers - 1, batch, W, gru_hid_dim), mask_rec (recon_n_layers - 1, batch, W, recon_hid_dim); either may be NULL. */
int mtadgat_dropout_masks_rnn(mtadgat_handle h, int64_t batch, int64_t window0, float dropout_p, uint64_t seed, float* mask_gru,
                              float* mask_rec, void* stream);
int mtadgat_train_layout(mtadgat_handle h, int64_t batch, int64_t* offsets_host, int max_n);

/* ---- anomaly-score post-processing on the device (callers' data path) ------
 * The arithmetic of Predictor.get_score (prediction.py:72-91) and of the threshold evaluation
 * (eval_methods.py: find_epsilon :189-236, adjust_predicts :6-55 + calc_point2point :58-72 for one threshold --
 * epsilon_eval -- or a whole sweep -- bf_search :117-158).  Device arrays in, small host tables out (these calls
 * synchronise the stream); the scalar bookkeeping on top is mtad-gat-pytorch_amd/evaluation.py.  Status 0 / -1
 * (bad argument) / -3 (HIP) / -5 (more anomaly segments than max_seg).
 * Scratch (device, need not be initialised): moments >= 2 doubles; epsilon_table >= 64 + 4*nz doubles (1 <= nz <= 64, halo >= 0:
 * the table starts at scratch_dev + 64 whatever nz is); point_adjust >= 7*n_thr doubles followed by 2*max_seg + 2 ints. */
int mtadgat_eval_scores(const float* preds_dev, const float* recons_dev, const float* actual_dev, int64_t n, int d,
                        int64_t ld_actual, const int* dims_dev, float gamma, float* per_dim_dev, float* global_dev, void* stream);
int mtadgat_eval_moments(const float* e_dev, int64_t n, double* scratch_dev, double* out_host, void* stream);
int mtadgat_eval_epsilon_table(const float* e_dev, int64_t n, const double* eps_host, int nz, int halo, double* scratch_dev,
                               double* out_host, void* stream);
int mtadgat_eval_point_adjust(const float* score_dev, const unsigned char* label_dev, int64_t n, const double* thr_host,
                              int n_thr, int compare_f32, int max_seg, double* scratch_dev, double* out_host, void* stream);
/* The two find_epsilon passes for every column of an (n, d) array with row stride ld >= d (floats) in one launch each.
 * moments: scratch >= 2*d doubles, out_host d x [sum, sumsq].  epsilon table: eps_host d x nz thresholds, scratch >= 5*d*nz
 * doubles, out_host d x nz x [pruned sum, pruned sumsq, pruned count, dilated count].  d <= 2048, nz <= 64. */
int mtadgat_eval_moments_columns(const float* e_dev, int64_t n, int d, int64_t ld, double* scratch_dev, double* out_host,
                                 void* stream);
int mtadgat_eval_epsilon_table_columns(const float* e_dev, int64_t n, int d, int64_t ld, const double* eps_host, int nz,
                                       int halo, double* scratch_dev, double* out_host, void* stream);
/* Quantiles of every column of a (n, d, ld) float32 array (prediction.py:84-88, --scale_scores): out_dev (nq, d) float32 in
 * np.percentile's "linear" definition -- pos = q (n - 1) in float64, lo = floor(pos), hi = min(lo + 1, n - 1),
 * s[lo] + (s[hi] - s[lo]) (pos - lo) evaluated in float64 from the two EXACT order statistics (radix select, no sort) and
 * rounded once.  A column holding a NaN gives NaN for every q.  Bitwise reproducible; asynchronous on `stream` (q_host is
 * read before the call returns).  n <= 2^31 - 1, d <= 2048, nq <= 4096, every q in [0, 1]; scratch_dev: 16-byte aligned,
 * at least mtadgat_eval_column_quantiles_scratch(n, d, nq) bytes (0 for invalid sizes), need not be initialised.
 * Status 0 / -1 (bad argument) / -3 (HIP) / -5 (scratch too small or misaligned); nothing is launched on an error. */
size_t mtadgat_eval_column_quantiles_scratch(int64_t n, int d, int nq);
int mtadgat_eval_column_quantiles(const float* a_dev, int64_t n, int d, int64_t ld, const double* q_host, int nq,
                                  void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream);
/* Exponentially weighted mean of a 1-D float32 array (pandas ewm(span).mean(), adjust=True; prediction.py:99-103,
 * --use_mov_av): alpha = 2 / (span + 1) in (0, 1], y[t] = N_t / D_t with N_t = x_t + (1 - alpha) N_{t-1} and
 * D_t = (1 - (1 - alpha)^(t + 1)) / alpha, a blocked scan in float64 with a fixed order of operations (bitwise
 * reproducible), stored as float32.  out_dev may be x_dev.  Asynchronous on `stream`.  scratch_dev: 8-byte aligned, at least
 * mtadgat_eval_ewm_scratch(n) bytes, need not be initialised.  Status as above. */
size_t mtadgat_eval_ewm_scratch(int64_t n);
int mtadgat_eval_ewm(const float* x_dev, int64_t n, double alpha, void* scratch_dev, size_t scratch_bytes, float* out_dev,
                     void* stream);
/* ---- scores of a gappy series (csrc/mtadgat_evalmask.hip; the VALID select and the VALID exponentially weighted scan of
 * csrc/mtadgat_evalcol.hip; evaluation.scored_rows, anomaly_scores(age=), the skip_nan arguments) -- tests/score_mask_refs.py is
 * the specification ------------------------------------------------------------------------------------------------------------
 * A score exists exactly where mtadgat_fit_windows (below) would have drawn a training window: score i belongs to window start i
 * and target row i + W.  NaN means "no score": the calls here write the canonical quiet NaN 0x7fc00000 and skip every NaN
 * they read, whatever its sign or payload; +-inf is a value, not a gap.  Conventions of the two calls above: no atomics on
 * floating-point values, no library kernels, bitwise reproducible; status 0 / -1 / -3 / -5 with a mtadgat_last_error() message;
 * nothing is launched when validation fails; scratch need not be initialised.  n <= 2^31 - 1, d <= 2048.
 *
 * mtadgat_eval_mark_rows: keep_dev[i] (uint8, n entries) = 1 for i in starts_dev[0 .. *count_dev) and 0 elsewhere; the count is read
 * on the device (cut to [0, n]; a start outside [0, n) is ignored), so mtadgat_fit_windows followed by this call gives "which scores
 * exist" without a host read.  Asynchronous on `stream`.
 *
 * mtadgat_eval_scores_masked: mtadgat_eval_scores over observed samples.  age_dev points at the age row of score 0 (row W of the
 * series' (N, F) int32 ages, row stride ld_age) and is indexed by the same column -- dims_dev[k] or k -- as actual_dev; a target
 * sample is observed iff age <= max_age.  per_dim[i][k] is mtadgat_eval_scores' expression in its float32 arithmetic where the sample
 * is observed and keep_dev[i] != 0 (NULL: all kept), else NaN.  global[i] is the float32 sum over those entries in k order -- a
 * select, not a multiply: a NaN or inf of `actual` under the mask does not reach it -- divided by (float)count, NaN for count = 0;
 * count_dev[i] (int32, may be NULL) is their number.  per_dim_dev and global_dev may be NULL.  With everything observed and kept the
 * outputs equal mtadgat_eval_scores' bit for bit.  Asynchronous on `stream`.
 *
 * mtadgat_eval_row_means_valid: global_dev[i] = the float32 sum of the non-NaN entries of row i of a_dev, (n, d) with row stride ld,
 * in column order, divided by (float) their number; NaN for a row without one; count_dev[i] (int32, may be NULL) their number: the
 * mean of mtadgat_eval_scores_masked for per-dimension scores that were scaled after masking.  Asynchronous on `stream`.
 *
 * mtadgat_eval_column_quantiles_valid: mtadgat_eval_column_quantiles over the m non-NaN entries of each column
 * (np.nanpercentile(..., method="linear")): pos = q (m - 1), the two exact order statistics, float64 interpolation, rounded once;
 * m = 0 gives NaN.  A count pass leaves m per column on the device (integer sums, independent of their order), the select's ranks
 * are set per column from it, and every NaN takes the one key above +inf, which no rank below m reaches.  count_dev (d) int64,
 * may be NULL, receives m.  Limits, scratch alignment (16 bytes) and status of mtadgat_eval_column_quantiles.
 *
 * mtadgat_eval_ewm_valid: the exponentially weighted mean over observed rows; a NaN input is an unobserved row.  In float64, with
 * b = 1 - alpha: N_t = (obs ? x_t : 0) + b N_{t-1}, D_t = (obs ? 1 : 0) + b D_{t-1}, out[t] = float(N_t / D_t) at an observed row
 * (D_t >= 1 there: no 0 / 0) and NaN at an unobserved one -- pandas' ewm(span, adjust=True, ignore_na=False).mean() at the observed
 * rows; pandas repeats the previous mean at an unobserved row, here that row has no score.  A blocked scan on (N, D) pairs in a
 * fixed order; across a long gap b^gap may underflow to 0 and the history is forgotten, as in the sequential recursion.  out_dev
 * may be x_dev.  Scratch: 8-byte aligned, mtadgat_eval_ewm_valid_scratch(n) bytes.  Asynchronous on `stream`.
 *
 * mtadgat_eval_moments_valid: out_host (d, 3) float64 = per column the sum, the sum of squares and the count of the non-NaN entries
 * of an (n, d) array with row stride ld: per-block partials by a fixed tree, then one wave per column that adds them in block
 * order -- no atomics, two calls give the same bits (unlike mtadgat_eval_moments_columns).  Synchronises the stream.  Scratch: 8-byte
 * aligned, mtadgat_eval_moments_valid_scratch(n, d) bytes.
 * The z table needs no call of its own: mtadgat_eval_epsilon_table(_columns) compares x < eps and x >= eps, both false for a NaN, so
 * a missing row enters neither the pruned sums and count nor the hot flags; it IS counted in the dilated count when it lies inside
 * a hot row's halo. */
int mtadgat_eval_mark_rows(const int64_t* starts_dev, const int64_t* count_dev, int64_t n, uint8_t* keep_dev, void* stream);
int mtadgat_eval_scores_masked(const float* preds_dev, const float* recons_dev, const float* actual_dev, int64_t n, int d,
                               int64_t ld_actual, const int32_t* dims_dev, float gamma, const int32_t* age_dev, int64_t ld_age,
                               int32_t max_age, const uint8_t* keep_dev /* n or NULL */, float* per_dim_dev, float* global_dev,
                               int32_t* count_dev /* n or NULL */, void* stream);
int mtadgat_eval_row_means_valid(const float* a_dev, int64_t n, int d, int64_t ld, float* global_dev, int32_t* count_dev /* n or NULL */,
                                 void* stream);
size_t mtadgat_eval_column_quantiles_valid_scratch(int64_t n, int d, int nq);
int mtadgat_eval_column_quantiles_valid(const float* a_dev, int64_t n, int d, int64_t ld, const double* q_host, int nq,
                                        void* scratch_dev, size_t scratch_bytes, float* out_dev, int64_t* count_dev /* d or NULL */,
                                        void* stream);
size_t mtadgat_eval_ewm_valid_scratch(int64_t n);
int mtadgat_eval_ewm_valid(const float* x_dev, int64_t n, double alpha, void* scratch_dev, size_t scratch_bytes, float* out_dev,
                           void* stream);
size_t mtadgat_eval_moments_valid_scratch(int64_t n, int d);
int mtadgat_eval_moments_valid(const float* e_dev, int64_t n, int d, int64_t ld, void* scratch_dev, size_t scratch_bytes,
                               double* out_host /* (d, 3) */, void* stream);
/* ---- from thresholded scores to events (csrc/mtadgat_events.hip; evaluation.anomaly_events) ----------------------------
 * Conventions of the two calls above: no float atomics, no library kernels, nothing sorted, bitwise reproducible; scratch
 * is 8-byte aligned, at least what the _scratch function returns (0 for invalid sizes), and need not be initialised;
 * status 0 / -1 (bad argument) / -3 (HIP) / -5 (scratch too small or misaligned; more runs than max_runs), with a
 * mtadgat_last_error() message; nothing is launched when validation fails.  n <= 2^31 - 1, d <= 2048, indices are int64.
 *
 * The flag of sample i comes from exactly one source (the other pointer is NULL): score_dev -- flag = score_i > threshold,
 * compared in float64, or in float32 with compare_f32 (mtadgat_eval_point_adjust's convention); NaN and equality are not
 * flagged -- or label_dev (uint8): flag = label_i != 0, threshold and compare_f32 ignored.
 *
 * mtadgat_eval_runs: the maximal runs of flagged samples as [start, end), in ascending order.  Consecutive runs whose
 * separation start_{k+1} - end_k is at most merge_gap >= 0 are merged (this chains; the gap samples belong to the event),
 * then events with end - start < min_length (>= 1) are dropped.  start_dev / end_dev hold max_runs >= 1 entries; the true
 * count is written to *count_host and the call synchronises the stream.  A count above max_runs returns -5 with
 * *count_host set and the first max_runs events written: call again with that capacity.  mtadgat_eval_runs_chunk() is the
 * chunk length of the blocked scans behind it (for tests that want sizes around it). */
int mtadgat_eval_runs_chunk(void);
size_t mtadgat_eval_runs_scratch(int64_t n);
int mtadgat_eval_runs(const float* score_dev, const unsigned char* label_dev, int64_t n, double threshold, int compare_f32,
                      int64_t merge_gap, int64_t min_length, int64_t max_runs, void* scratch_dev, size_t scratch_bytes,
                      int64_t* start_dev, int64_t* end_dev, int64_t* count_host, void* stream);
/* mtadgat_eval_run_stats: reductions over `count` given runs [start_k, end_k) of score_dev (n) -- disjoint and ascending,
 * as mtadgat_eval_runs returns them; bounds are cut to [0, n].  Asynchronous on `stream`.
 *   peak_dev[k]        the smallest index attaining the maximum of the run's scores with NaN read as -inf (-1: empty run)
 *   peak_score_dev[k]  that maximum
 *   mean_score_dev[k]  the float64 sum over the run divided by end - start, stored as float32 (a NaN inside gives NaN)
 * With per_dim_dev, an (n, d) float32 array with row stride ld >= d (NULL: d, ld, top_k are ignored and the four outputs
 * below may be NULL):
 *   feature_means_dev  (count, d) the same mean per column
 *   top_idx_dev, top_val_dev  (count, top_k) the top_k columns by the stored float32 mean, descending, ties to the lower
 *                      column, NaN last; 1 <= top_k <= min(d, 64)
 * With thr_dev as well, (d) float64 on the device:
 *   feature_hits_dev   (count, d) int32: the run's rows with per_dim >= thr_j, compared in float64
 * The sums are float64 partials of fixed row blocks added in block order: the bits do not depend on the launch shape.
 * scratch: mtadgat_eval_run_stats_scratch(n, count, d) bytes, d = 0 without per_dim. */
size_t mtadgat_eval_run_stats_scratch(int64_t n, int64_t count, int d);
int mtadgat_eval_run_stats(const float* score_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                           const float* per_dim_dev, int d, int64_t ld, const double* thr_dev, int top_k, void* scratch_dev,
                           size_t scratch_bytes, int64_t* peak_dev, float* peak_score_dev, float* mean_score_dev,
                           float* feature_means_dev, int* top_idx_dev, float* top_val_dev, int* feature_hits_dev, void* stream);
/* mtadgat_eval_first_hit: first_dev[k] = the smallest index in [start_k, end_k) whose flag is set, or -1; one wave per run,
 * so long runs are fine.  Scores as the source and labelled segments as the runs: detection and latency per segment;
 * labels as the source and events as the runs: whether an event overlaps a label.  Asynchronous on `stream`. */
int mtadgat_eval_first_hit(const float* score_dev, const unsigned char* label_dev, int64_t n, double threshold, int compare_f32,
                           const int64_t* start_dev, const int64_t* end_dev, int64_t count, int64_t* first_dev, void* stream);

/* ---- series made of parts (csrc/mtadgat_parts.hip; evaluation.score_parts, adjust_part_scores, moving_average(parts=),
 * find_epsilon_parts, part_predictions) -------------------------------------------------------------------------------------
 * A series that is a concatenation of independent entities (the channels of MSL / SMAP, the machines of SMD), scored part by
 * part: what the reference's adjust_anomaly_scores (utils.py:210-255) does around the seams, and the moving average and
 * find_epsilon restarted per part.  tests/part_refs.py states the definitions in numpy.
 *
 * Conventions of the event calls above: no atomics, no library kernels, bitwise reproducible (float64 partials of fixed row
 * blocks added in block order: the bits do not depend on the launch shape); scratch is 8-byte aligned, at least what the
 * _scratch function returns (0 for invalid sizes), and need not be initialised; status 0 / -1 / -3 / -5 with a
 * mtadgat_last_error() message; nothing is launched when validation fails.  1 <= n <= 2^31 - 1, indices are int64.  The
 * number of launches does not depend on `count`.
 *
 * The parts are `count` >= 1 spans [start_k, end_k) of score indices on the device, disjoint and ascending (empty spans are
 * fine), bounds cut to [0, n].  The arrays live on the device, so this is the caller's promise and is not checked.  A score
 * that no span covers belongs to no part: adjust writes it through (blanked if transitional), the moving average gives NaN,
 * its flag is 0 and the moments and tables do not see it.
 *
 * mtadgat_eval_part_adjust: x_dev is (n, d) float32 with row stride ld >= d (1-D: d = ld = 1), d <= 2048; out_dev likewise with
 * ld_out.  A score i with t - before <= i <= t + after for one of the n_seams seams t (seam_dev, int64, ascending, on the
 * device; NULL with n_seams = 0) becomes +0.0 in every column.  With normalize, every (part, column) is then mapped to
 * (x - lo) / (hi - lo), evaluated in float64 and rounded once, lo / hi being the minimum / maximum of its non-NaN values after
 * blanking; NaN stays NaN, +-inf are ordinary values, and where hi <= lo (a constant, all-NaN or empty part) every non-NaN value
 * becomes +0.0.  lohi_dev (NULL, or (count, d, 2) float64 on the device, only with normalize) receives lo and hi (+inf and -inf
 * where the part has no non-NaN value).  Without normalize only the blanking is done and scratch may be NULL.  out_dev may be
 * x_dev itself (with ld_out = ld), and must not overlap it otherwise.  Asynchronous on `stream`, nothing is read back.
 *
 * mtadgat_eval_ewm_parts: mtadgat_eval_ewm restarted at every span start: inside span [s, e) N_t = x_t + (1 - alpha) N_{t-1}
 * with N_{s-1} = 0, D_t = (1 - (1 - alpha)^(t - s + 1)) / alpha, y_t = N_t / D_t.  The scan carries (sum, "a span started")
 * pairs, so no part's sum is ever subtracted from a later one; with one span [0, n) the bits are mtadgat_eval_ewm's (the two are
 * instantiations of one scan, csrc/mtadgat_evalcol.hip).
 * out_dev may be x_dev.  Asynchronous on `stream`.
 *
 * mtadgat_eval_part_epsilon_moments / _table: the two device passes of find_epsilon for every part at once, each ending in one
 * small copy to the host (they synchronise the stream).  moments: out_host count x [sum, sum of squares, maximum] (0, 0, -inf
 * for an empty part; the maximum is NaN if the part holds a NaN).  table: eps_host count x nz thresholds (1 <= nz <= 64),
 * out_host count x nz x [pruned sum, pruned sum of squares, pruned count, dilated count] as mtadgat_eval_epsilon_table defines
 * them (one tile routine computes both, csrc/mtadgat_scan.h), the +-halo dilation (0 <= halo <= 128) never looking outside the
 * part.  Both take the same scratch,
 * mtadgat_eval_part_epsilon_scratch(n, count, nz).
 *
 * mtadgat_eval_part_flags: flags_dev[i] (uint8) = x_i > thr_dev[part(i)], thr_dev (count) float64 on the device, compared in
 * float64; NaN and equality are not flagged.  Asynchronous on `stream`.
 *
 * mtadgat_eval_part_quantiles: np.percentile(a[start_k : end_k], 100 q, axis=0) ("linear") for every part k of a_dev, (n, d) float32
 * with row stride ld >= d, d <= 2048, and the nq probabilities q_host (1 <= nq <= 8, each in [0, 1]; they travel in the kernel
 * arguments: no copy, q_host is free on return).  out_dev is (nq, count, d) float32.  Per (part, column) the semantics are
 * mtadgat_eval_column_quantiles' with the part's length: the two order statistics each probability needs are exact (a
 * most-significant-digit radix select on the order bits, nothing is sorted), interpolated in float64 and rounded once; a (part,
 * column) that holds a NaN gives NaN for every q and touches no other; an empty part gives NaN, a part of one row that row.
 * Histogram bins are integer atomics (integer sums do not depend on their order), there are no float atomics: bitwise
 * reproducible.  A part of at most mtadgat_eval_partq_long() rows is selected inside one workgroup, its bins never leaving LDS;
 * a longer one runs the passes of mtadgat_eval_column_quantiles restricted to its rows, its bins in scratch slot
 * floor(start / mtadgat_eval_partq_long()).  Scratch (16-byte aligned, need not be initialised) is
 * (n / partq_long + 1) d 2 nq KiB of bins and select state (none for n <= partq_long) plus 8 nq + 4 bytes per (part, column).
 * Asynchronous on `stream`.
 *
 * mtadgat_eval_part_scale: out[i, c] = (a[i, c] - median) / (1 + (q75 - q25)) with q_dev (3, count, d) float32 = q25, median, q75
 * of the part that owns row i, as mtadgat_eval_part_quantiles writes them for q = 0.25, 0.5, 0.75.  float32, every operation
 * rounded on its own.  A row that no span covers gives NaN.  out_dev (row stride ld_out >= d) may be a_dev itself (with
 * ld_out = ld), and must not overlap it otherwise.  One launch, no scratch, asynchronous on `stream`. */
size_t mtadgat_eval_part_quantiles_scratch(int64_t n, int d, int64_t count, int nq);
int mtadgat_eval_part_quantiles(const float* a_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev,
                                int64_t count, const double* q_host, int nq, void* scratch_dev, size_t scratch_bytes,
                                float* out_dev /* (nq, count, d) */, void* stream);
int mtadgat_eval_partq_long(void);
int mtadgat_eval_part_scale(const float* a_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev,
                            int64_t count, const float* q_dev /* (3, count, d) */, float* out_dev, int64_t ld_out, void* stream);
size_t mtadgat_eval_part_adjust_scratch(int64_t n, int d, int64_t count);
int mtadgat_eval_part_adjust(const float* x_dev, int64_t n, int d, int64_t ld, const int64_t* start_dev, const int64_t* end_dev,
                             int64_t count, const int64_t* seam_dev, int64_t n_seams, int64_t before, int64_t after, int normalize,
                             void* scratch_dev, size_t scratch_bytes, float* out_dev, int64_t ld_out, double* lohi_dev, void* stream);
size_t mtadgat_eval_ewm_parts_scratch(int64_t n);
int mtadgat_eval_ewm_parts(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count, double alpha,
                           void* scratch_dev, size_t scratch_bytes, float* out_dev, void* stream);
size_t mtadgat_eval_part_epsilon_scratch(int64_t n, int64_t count, int nz);
int mtadgat_eval_part_epsilon_moments(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                                      int nz, void* scratch_dev, size_t scratch_bytes, double* out_host, void* stream);
int mtadgat_eval_part_epsilon_table(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                                    const double* eps_host, int nz, int halo, void* scratch_dev, size_t scratch_bytes,
                                    double* out_host, void* stream);
int mtadgat_eval_part_flags(const float* x_dev, int64_t n, const int64_t* start_dev, const int64_t* end_dev, int64_t count,
                            const double* thr_dev, unsigned char* flags_dev, void* stream);

/* ---- squared errors of windows against their series (csrc/mtadgat_losses.hip; evaluation.window_sse) ---------------------
 * What the reference's Trainer.evaluate (training.py:188-228) reduces model(x) to.  Conventions of the part calls above: no
 * atomics, bitwise reproducible, status 0 / -1 / -3 / -5 with a mtadgat_last_error() message, nothing touches the device when
 * validation fails, asynchronous on `stream`.
 *
 * mtadgat_eval_window_sse: for window w of the call, first row s_w = starts_dev[w] or start0 + w * stride of series_dev
 * ((n_rows, F) float32, row stride ld_series >= F), and column dims_dev[d] (NULL: d) for output dimension d:
 *   window_sse_dev[w, 0] = sum_d        (preds_dev[w, d]     - series[s_w + W, dims[d]])^2
 *   window_sse_dev[w, 1] = sum_{t < W} sum_d (recons_dev[w, t, d] - series[s_w + t, dims[d]])^2
 *   dim_sse_dev[0, d], dim_sse_dev[1, d]   the same squares summed over the windows (and time steps) instead of over d
 * Every difference is ONE float32 subtraction (numpy's float32 a - b), converted to float64 and squared there -- exact -- and
 * the squares are summed in float64 in a fixed order.  A window's pair depends on that window's data alone.  The per-dimension
 * sums are a two-stage reduction (per-slab partials, then one wave per entry); their bits depend on the inputs and on how the
 * caller cut the windows into calls, on nothing else.  accumulate = 0: the per-dimension sums start at 0; 1: they continue the
 * sums the previous call with a non-NULL dim_sse_dev left in the SAME scratch (any batch whose scratch need is not larger), and
 * dim_sse_dev receives the total so far.  dim_sse_dev may be NULL: only window_sse_dev is written.
 * Limits: 1 <= batch <= 2^31 - 1, 1 <= out_dim <= 2048, 1 <= W <= 512, ld_series >= F >= 1, out_dim <= F when dims_dev is NULL,
 * n_rows >= W + 1.  With starts_dev NULL the progression is checked on the host: start0 >= 0, stride >= 0 and
 * start0 + (batch - 1) stride + W <= n_rows - 1 (the target row exists); starts_dev and dims_dev are the caller's to check.
 * Scratch: 16-byte aligned, at least mtadgat_eval_window_sse_scratch(batch, out_dim) bytes (0 for refused sizes; non-decreasing
 * in batch), need not be initialised for accumulate = 0.
 *
 * mtadgat_eval_group_sums: out_dev[g, c] = sum of x_dev[i, c] over the rows i of group g = [g group, min((g + 1) group, n)) of
 * x_dev (n, cols) float64 -- ceil(n / group) groups, the last one may be short --, in float64 in a fixed order.
 * 1 <= n <= 2^31 - 1, 1 <= cols <= 64, group >= 1. */
size_t mtadgat_eval_window_sse_scratch(int64_t batch, int out_dim);
int mtadgat_eval_window_sse(const float* preds_dev /* (batch, out_dim) */, const float* recons_dev /* (batch, W, out_dim) */,
                            int64_t batch, int W, int out_dim, const float* series_dev, int64_t n_rows, int F, int64_t ld_series,
                            const int64_t* starts_dev, int64_t start0, int64_t stride, const int32_t* dims_dev, int accumulate,
                            double* window_sse_dev /* (batch, 2) */, double* dim_sse_dev /* (2, out_dim) or NULL */,
                            void* scratch_dev, size_t scratch_bytes, void* stream);
int mtadgat_eval_group_sums(const double* x_dev, int64_t n, int cols, int64_t group, double* out_dev /* (groups, cols) */,
                            void* stream);

/* ---- an optimisation step on windows of a device-resident series (csrc/mtadgat_fit.hip; fitting.SeriesTrainer) -------------
 * What surrounds mtadgat_forward_train / mtadgat_backward in a step of the reference's Trainer.fit (training.py:100-130): the
 * window gather, the cotangents of sqrt(mse) + sqrt(mse), the gradient norm with the step's set-up, Adam.  tests/fit_refs.py is
 * the specification.  Conventions of the calls above: handle-free, no atomics, identical calls give identical bits, status
 * 0 / -1 / -3 / -5 with a mtadgat_last_error() message, nothing touches the device when validation fails, asynchronous on
 * `stream`, no stream synchronisation.  starts_dev and dims_dev are the caller's to check, as in mtadgat_eval_window_sse.
 *
 * mtadgat_fit_gather: x_dev[w, t, :] = series_dev[starts_dev[w] + t, 0:F] for t < W; series_dev (n_rows, F) float32 with row
 * stride ld_series >= F (rows need not be 16-byte aligned), x_dev (batch, W, F) contiguous.  1 <= batch <= 2^31 - 1,
 * 1 <= W <= 512, 1 <= F <= 2048, n_rows >= W.
 *
 * mtadgat_fit_loss_grad: the cotangents of loss = rmse_f + rmse_r of one batch.  sums_dev[0], sums_dev[1] are the batch's two
 * squared-error sums: mtadgat_eval_window_sse followed by mtadgat_eval_group_sums(group = batch) over its (batch, 2) output.
 * With N_f = batch out_dim, N_r = batch W out_dim, in float64: rmse = sqrt(S / N), c = 1 / (N rmse);
 *   d_preds_dev[w, d]     = float(double(preds_dev[w, d]     - series[s_w + W, dims[d]]) c_f)
 *   d_recons_dev[w, t, d] = float(double(recons_dev[w, t, d] - series[s_w + t, dims[d]]) c_r)
 * each difference the ONE float32 subtraction of mtadgat_eval_window_sse; rmse_dev[0] = rmse_f, rmse_dev[1] = rmse_r.
 * Departure from torch: rmse == 0 (every residual of the head is 0) gives c = 0, a zero cotangent, where autograd's sqrt gives
 * 0 / 0.  A sum that is not finite gives c = NaN: every cotangent of that head is NaN.  Limits of mtadgat_eval_window_sse.
 *
 * mtadgat_fit_prepare: the squared norm of grads_dev (n floats) as a float64 sum of double(g)^2 in a fixed order -- blocks of
 * 4096 consecutive entries, in a block lane t of 256 adds entries t, t + 256, .. from +0.0 and the lanes meet in the halving
 * tree of mtadgat_eval_group_sums; the blocks' sums are added the same way -- and from it the step record state_dev, 8 float64:
 *   [0] t            steps applied so far; this call adds 1 when it applies
 *   [1] calls        calls so far (applied or not); this call adds 1
 *   [2] clip         min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_), 1 for max_norm < 0: no clipping
 *   [3] step_size    lr / (1 - beta1^t)         b^t by squaring: r = 1; while t: (t odd: r *= b); b *= b; t >>= 1
 *   [4] bc2s         sqrt(1 - beta2^t)
 *   [5] applied      1, or 0 when skip_nonfinite is set and the norm, rmse_dev[0] or rmse_dev[1] is not finite: t and fields
 *                    [2] .. [4] then stay as they were and mtadgat_fit_adam writes nothing
 *   [6] norm^2  [7] norm
 * The caller zeroes the record before the first step; it is all of the optimiser's scalar state.  Row (calls mod capacity) of
 * log_dev (capacity, 4) float64 receives (rmse_f, rmse_r, norm, applied), `calls` counted before this call.
 * Scratch: 8-byte aligned, mtadgat_fit_prepare_scratch(n) bytes (0 for a refused n), need not be initialised.
 * lr finite and >= 0, betas in [0, 1), 1 <= capacity <= 2^31 - 1.
 *
 * mtadgat_fit_adam: Adam over the flat float32 buffers, per element in float64 with every product rounded (no fused
 * multiply-add), (clip, step_size, bc2s, applied) from state_dev:
 *   g' = g clip (+ weight_decay p);   decoupled: p' = p (1 - lr weight_decay) instead (AdamW)
 *   m <- beta1 m + (1 - beta1) g';   v <- beta2 v + (1 - beta2) (g' g');   p <- p' - step_size (m / (sqrt(v) / bc2s + eps))
 * p, m and v are each stored with ONE rounding to float32.  torch.optim.Adam does the same algebra in float32, rounding after
 * every operation: its parameters differ from these in the last bits.  eps, weight_decay finite and >= 0. */
#define MTADGAT_FIT_STATE_FIELDS 8
int mtadgat_fit_gather(const float* series_dev, int64_t n_rows, int F, int64_t ld_series, const int64_t* starts_dev, int64_t batch,
                       int W, float* x_dev /* (batch, W, F) */, void* stream);
int mtadgat_fit_loss_grad(const float* preds_dev /* (batch, out_dim) */, const float* recons_dev /* (batch, W, out_dim) */,
                          int64_t batch, int W, int out_dim, const float* series_dev, int64_t n_rows, int F, int64_t ld_series,
                          const int64_t* starts_dev, const int32_t* dims_dev, const double* sums_dev /* 2 */, float* d_preds_dev,
                          float* d_recons_dev, double* rmse_dev /* 2 */, void* stream);
size_t mtadgat_fit_prepare_scratch(int64_t n);
int mtadgat_fit_prepare(const float* grads_dev, int64_t n, const double* rmse_dev /* 2 */, double lr, double beta1, double beta2,
                        double max_norm, int skip_nonfinite, double* state_dev /* MTADGAT_FIT_STATE_FIELDS */,
                        double* log_dev /* (capacity, 4) */, int64_t capacity, void* scratch_dev, size_t scratch_bytes, void* stream);
int mtadgat_fit_adam(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                     const double* state_dev, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                     void* stream);

/* ---- training on gappy, concatenated series (csrc/mtadgat_fitwin.hip, _losses.hip, _fit.hip; fitting.training_windows) -------
 * The window sampler and the losses that count observed samples only.  tests/fit_mask_refs.py is the specification.
 * Conventions of the fit calls above.  age_dev: (n_rows, F) int32 with row stride ld_age >= F, as the preparation's transform
 * reports it -- 0 for a real sample, k for the k-th consecutive filled row; a sample is OBSERVED iff age <= max_age.
 *
 * mtadgat_fit_windows: the window starts a trainer may draw from.  Start s in [0, n_rows - W) reads rows s .. s + W - 1 and is asked
 * for row s + W; it is valid iff
 *   1. rows s .. s + W lie in one part: part p is rows [part_offsets_dev[p], part_offsets_dev[p + 1]), `parts` + 1 ascending int64
 *      offsets from 0 to n_rows (NULL: one part);
 *   2. row s + W has at least one observed sample among the columns dims_dev[0 .. out_dim) (NULL: 0 .. out_dim - 1);
 *   3. rows s .. s + W - 1 hold at least min_count observed samples over all F columns.
 * starts_dev[0 .. count) receives the valid starts in ascending order, *count_dev their number; entries from count on are not
 * written.  age_dev NULL: every sample is observed.  All integer arithmetic, no atomics; seven launches whatever `parts` is (the
 * part of a start is a binary search in the offsets); identical calls give identical bits.  Limits of mtadgat_fit_gather,
 * 1 <= out_dim <= 2048 (<= F when dims_dev is NULL), W <= n_rows <= 2^31 - 1, 1 <= parts <= 2^31 - 1, min_count >= 0.  The offsets and
 * dims_dev are the caller's to check.  Scratch: 8-byte aligned, mtadgat_fit_windows_scratch(n_rows) bytes (0 for a refused n_rows),
 * need not be initialised; short or misaligned scratch is refused with -5 before anything is launched.
 *
 * mtadgat_fit_masked_sse: mtadgat_eval_window_sse over observed samples only.  window_dev[w] = (S_f, S_r, N_f, N_r): S is that
 * call's sum with every unobserved term replaced by +0.0 -- a select, a NaN under the mask does not reach the sum --, added in that
 * call's order, so with everything observed S equals its sums bit for bit; N counts the observed terms (float64, exact).
 * dim_dev (4, out_dim) or NULL: the same four per output dimension over the call's windows, with mtadgat_eval_window_sse's slab
 * scheme and its `accumulate`.  Its limits.  Scratch: 16-byte aligned, mtadgat_fit_masked_sse_scratch(batch, out_dim) bytes.
 * mtadgat_eval_group_sums(cols = 4, group = batch) over window_dev gives the batch's four sums.
 *
 * mtadgat_fit_masked_loss_grad: mtadgat_fit_loss_grad from those four sums, sums_dev = (S_f, S_r, N_f, N_r).  Per head in float64:
 * rmse = sqrt(S / N) for N > 0, else 0;  c = NaN if S is not finite, 0 if N == 0 or rmse == 0, else 1 / (N rmse).  An observed
 * entry receives float(double(df) c) with df the ONE float32 subtraction, an unobserved one +0.0f whatever c is; rmse_dev
 * receives the two rmse. */
size_t mtadgat_fit_windows_scratch(int64_t n_rows);
int mtadgat_fit_windows(const int32_t* age_dev /* (n_rows, F) or NULL */, int64_t ld_age, int32_t max_age, int64_t n_rows, int F, int W,
                        const int32_t* dims_dev /* out_dim or NULL */, int out_dim, const int64_t* part_offsets_dev /* parts + 1 or NULL */,
                        int64_t parts, int64_t min_count, int64_t* starts_dev /* capacity n_rows - W */, int64_t* count_dev /* 1 */,
                        void* scratch_dev, size_t scratch_bytes, void* stream);
size_t mtadgat_fit_masked_sse_scratch(int64_t batch, int out_dim);
int mtadgat_fit_masked_sse(const float* preds_dev /* (batch, out_dim) */, const float* recons_dev /* (batch, W, out_dim) */, int64_t batch,
                           int W, int out_dim, const float* series_dev, int64_t n_rows, int F, int64_t ld_series,
                           const int64_t* starts_dev, int64_t start0, int64_t stride, const int32_t* dims_dev, const int32_t* age_dev,
                           int64_t ld_age, int32_t max_age, int accumulate, double* window_dev /* (batch, 4) */,
                           double* dim_dev /* (4, out_dim) or NULL */, void* scratch_dev, size_t scratch_bytes, void* stream);
int mtadgat_fit_masked_loss_grad(const float* preds_dev /* (batch, out_dim) */, const float* recons_dev /* (batch, W, out_dim) */,
                                 int64_t batch, int W, int out_dim, const float* series_dev, int64_t n_rows, int F, int64_t ld_series,
                                 const int64_t* starts_dev, const int32_t* dims_dev, const int32_t* age_dev, int64_t ld_age,
                                 int32_t max_age, const double* sums_dev /* 4 */, float* d_preds_dev, float* d_recons_dev,
                                 double* rmse_dev /* 2 */, void* stream);

/* ---- ranking curves (csrc/mtadgat_curves.hip; evaluation.score_order, ranking_curve, ranking_metrics) -------------------
 * Conventions of the event calls above: no atomics, no library kernels, bitwise reproducible; scratch is 8-byte aligned, at
 * least what the _scratch function returns (0 for invalid sizes) and need not be initialised; status 0 / -1 / -3 / -5 with a
 * mtadgat_last_error() message; nothing is launched when validation fails.  1 <= n <= 2^31 - 1.
 *
 * mtadgat_eval_order_key (host): the 32-bit key whose unsigned order is the rank order of float32 values: -0.0 is read as
 * +0.0, the sign bit is flipped for non-negative values and all bits for negative ones, the result is inverted when
 * `descending`; every NaN gives 0xffffffff, the largest key, in both directions.
 * mtadgat_eval_sort_tile(): the items per tile of the radix sort behind the calls below; mtadgat_eval_sort_scan_tiles(): the number
 * of tiles above which the sort's (digit, tile) scan takes a second level (for tests that want sizes around both). */
uint32_t mtadgat_eval_order_key(float value, int descending);
int mtadgat_eval_sort_tile(void);
int mtadgat_eval_sort_scan_tiles(void);
/* mtadgat_eval_score_order: order_dev[r] = the index of the score of rank r, by ascending order key (see above) for the given
 * direction; equal keys keep ascending index (a stable least-significant-digit radix sort, 8 bits per pass, 4 passes).
 * Asynchronous on `stream`. */
size_t mtadgat_eval_score_order_scratch(int64_t n);
int mtadgat_eval_score_order(const float* score_dev, int64_t n, int descending, void* scratch_dev, size_t scratch_bytes,
                             int64_t* order_dev, void* stream);
/* mtadgat_eval_curve: every operating point of score_dev (n float32) against label_dev (n uint8, != 0 is positive).
 * adjust 0: the scores as they are; 1: point adjust -- every sample of a labelled segment takes the segment's largest non-NaN
 * score, except that sample 0 keeps its own (mtadgat_eval_point_adjust's back-fill never reaches index 0); 2: PA%K with
 * 0 <= k_percent <= 100 -- a sample of a segment of length L takes max(own, the m-th largest non-NaN score of the segment),
 * m = k_percent * L / 100 + 1 (integer division), and keeps its own when the segment has fewer than m non-NaN scores.
 * thresholds_dev / tp_dev / fp_dev hold n entries each; the first G are written: the distinct non-NaN adjusted values in
 * descending order (never -0.0) and the numbers of positives / negatives with adjusted score >= that value.  A NaN is below
 * every threshold.  summary_host receives 12 int64 and the call synchronises the stream:
 *   [0] G  [1] positives  [2] negatives  [3] positives with a NaN adjusted score  [4] negatives with one
 *   [5] the doubled AUROC numerator: sum over the tie groups, the NaN samples being one last group, of
 *       (positives of the group) x (2 x negatives below the group + negatives of the group)
 *   [6] the bits of the float64 sum over the numeric groups of (positives of the group) x tp / (tp + fp), added in a fixed
 *       order whose longest chain of additions has at most 4096 terms
 *   [7] the group of largest F1 = 2 p r / (p + r + 1e-5), p = tp / (tp + fp + 1e-5), r = tp / (tp + fn + 1e-5), evaluated
 *       in float64 without contraction, the lowest group among equals, -1 when G = 0; [8], [9] its tp and fp; [10] the bits
 *       of its float32 threshold; [11] 0.
 * With adjust != 0 the number of labelled segments is read back as well (mtadgat_eval_runs), with adjust = 2 also the number
 * of labelled samples.  scratch: mtadgat_eval_curve_scratch(n, adjust) bytes. */
size_t mtadgat_eval_curve_scratch(int64_t n, int adjust);
int mtadgat_eval_curve(const float* score_dev, const unsigned char* label_dev, int64_t n, int adjust, int k_percent,
                       void* scratch_dev, size_t scratch_bytes, float* thresholds_dev, int64_t* tp_dev, int64_t* fp_dev,
                       int64_t* summary_host, void* stream);

/* ---- scoring live streams row by row (csrc/mtadgat_stream.hip; streaming.StreamScorer) ---------------------------------
 * A deployment's loop: rows of n_streams independent series arrive a few at a time, and each needs its anomaly score, an alarm
 * flag and -- when an alarm ends -- the finished event.  Everything that carries over from one push to the next lives in ONE
 * device allocation of mtadgat_stream_state_bytes() bytes (16-byte aligned) that the host never reads: per stream its row
 * counter, the last W + max_block - 1 rows (a ring stored twice, so that every window is contiguous; the rings of all streams
 * form one flat series for mtadgat_forward_series), the forecast pending for its next row, the moving-average state and the
 * open event.  Scores, indices and events are in the score-index space of Predictor.get_score (prediction.py:65-91): score
 * i of a stream belongs to its row i + W, the first row with both a full window behind it and a forecast from the row before;
 * rows 0 .. W - 1 give NaN scores and no flag.
 *   per_dim[d] = |forecast[d] - x[d]| + gamma |recon_last[d] - x[d]| in float64, optionally (. - center[d]) / (1 + spread[d])
 *   score      = the float64 mean over d, rounded once to float32; with alpha in (0, 1] the moving average of those float32
 *                scores (pandas ewm(span).mean(), alpha = 2 / (span + 1), adjust=True: N_t = x_t + (1 - alpha) N_{t-1},
 *                D_t = 1 + (1 - alpha) D_{t-1} in float64, N_t / D_t stored as float32); alpha = 0: no smoothing
 *   flag       = (double)score > threshold (NaN and equality are not flagged): `threshold`, or thresholds_dev[stream] when
 *                thresholds_dev, (n_streams) float64 on the device, is given
 *   events     = mtadgat_eval_runs' semantics, incrementally: flagged runs at most merge_gap apart merge, events shorter than
 *                min_length are dropped.  An event whose last flagged sample is e - 1 becomes final at sample e + merge_gap
 *                if nothing from e on was flagged, and is reported AT that sample: at most one per stream and sample.
 * Outputs of a push of T rows for n streams, each (n, T) in (stream, t) order and each optional (NULL): scores float32,
 * flags uint8, per_dim (n, T, d) float32, and the event that closed at the sample -- closed_start (-1: none), closed_end
 * (exclusive), closed_peak (the first index of the largest score) int64, closed_peak_score, closed_mean (float64 sum / length)
 * float32.  No atomics: the bits depend on the data and on the order of pushes per stream, not on how rows are cut into pushes.
 *
 * streams_dev: (n) distinct int64 stream indices on the device, or NULL for streams 0 .. n - 1; an index outside
 * [0, n_streams) gets "nothing" outputs and touches no state.  rows_dev (n, T, F) float32, T <= max_block.  n_streams and
 * max_block must be those of mtadgat_stream_init (the kernels refuse a state initialised for another geometry).  Nothing
 * synchronises except mtadgat_stream_init (it copies the three host vectors).  Status as everywhere. */
typedef struct mtadgat_stream_outputs {
    float*   scores;
    uint8_t* flags;
    float*   per_dim;
    int64_t* closed_start;
    int64_t* closed_end;
    int64_t* closed_peak;
    float*   closed_peak_score;
    float*   closed_mean;
} mtadgat_stream_outputs;
size_t mtadgat_stream_state_bytes(mtadgat_handle h, int64_t n_streams, int64_t max_block);
/* Zeroes the state.  dims_host (out_dim) int32: the series column of each output dimension, or NULL for 0 .. out_dim - 1
 * (needs out_dim == n_features); center_host / spread_host (out_dim) float32, both or neither. */
int mtadgat_stream_init(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, double gamma, double alpha,
                        int64_t merge_gap, int64_t min_length, const int32_t* dims_host, const float* center_host,
                        const float* spread_host, void* stream);
/* Workspace of mtadgat_stream_push for n * T = windows: the forward's, the window starts and the two model outputs --
 * preds (windows, out_dim) at its beginning, recons_last (windows, out_dim) right behind. */
size_t mtadgat_stream_workspace_bytes(mtadgat_handle h, int64_t windows);
/* The stage kernel, ONE mtadgat_forward_series over the flat history (preds and recons_last only) and the score kernel.
 * out == NULL stops after the forward: the rows are in the history and the model outputs in the workspace, but no counter
 * has moved, so the call can be repeated (re-packed weights) -- mtadgat_stream_update with staged = 1 then commits it. */
int mtadgat_stream_push(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, const float* rows_dev,
                        const int64_t* streams_dev, int64_t n, int64_t T, double threshold, const double* thresholds_dev,
                        const mtadgat_stream_outputs* out, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The stage and score kernels with the model outputs of the windows ending at the new rows supplied by the caller, (n, T,
 * out_dim) each: the state machine without a model in the way.  staged != 0: the rows are in the history already. */
int mtadgat_stream_update(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, const float* preds_dev,
                          const float* recons_last_dev, const float* rows_dev, const int64_t* streams_dev, int64_t n, int64_t T,
                          int staged, double threshold, const double* thresholds_dev, const mtadgat_stream_outputs* out, void* stream);
/* The still-open event of each selected stream, its end at the last flagged sample + 1, in the closed_* fields of `out` ((n)
 * each; may be NULL with reset); the state is left as it is unless reset != 0, which returns those streams to their state
 * after mtadgat_stream_init (history zeroed). */
int mtadgat_stream_flush(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, const int64_t* streams_dev,
                         int64_t n, int reset, const mtadgat_stream_outputs* out, void* stream);
/* Host only: the first slot, within a stream's 2R ring slots, of the window ending at the stream's row count + t -- the
 * function the stage kernel calls.  R = W + max_block - 1; -1 for count < 0, t < 0, W < 1 or R < W. */
int64_t mtadgat_stream_window_start(int64_t count, int64_t t, int64_t W, int64_t R);

/* ---- adaptive peaks-over-threshold thresholds (csrc/mtadgat_spot.hip, csrc/mtadgat_spot.h; evaluation.spot_*) ------------
 * SPOT (Siffer et al., KDD 2017) per column of a score matrix: each column keeps an initial threshold t, its excesses x - t over
 * it, and the alarm threshold z at the q-quantile of a generalized Pareto tail fitted to those excesses.  The definition of the
 * fit (candidates, root search, choice, threshold) is spelled out in csrc/mtadgat_spot.h; it follows the paper, not the
 * reference's spot.py, and tests/spot_refs.py is its specification.  One state allocation of mtadgat_spot_state_bytes() bytes
 * (16-byte aligned) holds, per column, (t, z, n, Nt, gamma, sigma) and a ring of the most recent max_peaks excesses.  The ring
 * is this library's own bound: Nt counts every excess, the fit sees only the stored ones -- until a ring wraps this is the
 * paper's Algorithm 1.  All arithmetic is float64; one wave fits one column; no atomics; bitwise reproducible.
 *
 * The step for one score x: the threshold reported for the row is z before the step; a NaN changes nothing and is not
 * flagged; x > z is flagged (and, when the state is dynamic, leaves it alone: alarms are not absorbed); otherwise a dynamic
 * state with x > t pushes x - t into the ring (dropping the oldest when full), increments Nt and n, refits and takes the new z,
 * and any other x increments n.  A static state (dynamic = 0) never changes.
 *
 * Refused with a message before anything is launched: q or level outside (0, 1), max_peaks outside [8, 4096], n_init < 16. */
size_t mtadgat_spot_state_bytes(int64_t n_columns, int64_t max_peaks);          /* 0 for sizes that are refused */
size_t mtadgat_spot_calibrate_scratch(int64_t n_init, int64_t n_columns);
/* Calibrates every column of init_dev (n_init, n_columns) float32, row stride ld: t = sorted[int(level * n_init)] (exact radix
 * select), the excesses in row order (the last max_peaks of them are kept), the first fit.  At most 65536 columns per call.
 * Synchronises the stream: a column with fewer than 8 excesses, a NaN or a non-positive mean excess fails the call with -1 and
 * a message naming the column. */
int mtadgat_spot_calibrate(const float* init_dev, int64_t n_init, int64_t n_columns, int64_t ld, double q, double level,
                           int64_t max_peaks, int dynamic, void* state_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
/* The step over the rows of scores_dev (n, n_columns) float32, row stride ld, in order: thresholds_dev (n, n_columns) float64
 * and flags_dev (n, n_columns) uint8, either may be NULL.  The state is left advanced, so a second call continues where the
 * first stopped.  Asynchronous.  A state calibrated for other sizes gives NaN thresholds, no flags, and is not touched. */
int mtadgat_spot_run(void* state_dev, int64_t n_columns, int64_t max_peaks, const float* scores_dev, int64_t n, int64_t ld,
                     double* thresholds_dev, uint8_t* flags_dev, void* stream);
/* out_host (n_columns, 6) float64: t, z, n, Nt, gamma, sigma per column.  Synchronises the stream. */
int mtadgat_spot_read(const void* state_dev, int64_t n_columns, int64_t max_peaks, double* out_host, void* stream);
/* Columns columns_dev[0 .. n) (NULL: 0 .. n - 1) of dst <- the same columns of src, or src's only column when src_columns is 1.
 * init != 0: dst is a fresh allocation that also takes src's header; then all its columns are copied (n = dst_columns, no
 * selection).  Asynchronous. */
int mtadgat_spot_copy(void* dst_dev, int64_t dst_columns, const void* src_dev, int64_t src_columns, int64_t max_peaks,
                      const int64_t* columns_dev, int64_t n, int init, void* stream);
/* Host only, no GPU needed: the fit over m >= 1 positive excesses (oldest first) for n observations, Nt excesses, initial
 * threshold t and risk q, with the sums taken in the order a wave takes them.  out_host[3] = gamma, sigma, z. */
int mtadgat_spot_fit_host(const double* peaks_host, int64_t m, int64_t n, int64_t Nt, double t, double q, double* out_host);
/* mtadgat_stream_push / _update with each stream compared against ITS column of a SPOT state of n_streams columns (a second
 * device allocation beside the stream state), after the smoothing; the column advances with the stream.  thresholds_out_dev:
 * (n, T) float64, what each row was compared against (NaN for a stream's first W rows), or NULL. */
int mtadgat_stream_push_spot(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, const float* rows_dev,
                             const int64_t* streams_dev, int64_t n, int64_t T, void* spot_dev, int64_t max_peaks,
                             double* thresholds_out_dev, const mtadgat_stream_outputs* out, void* workspace_dev, size_t workspace_bytes,
                             void* stream);
int mtadgat_stream_update_spot(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, const float* preds_dev,
                               const float* recons_last_dev, const float* rows_dev, const int64_t* streams_dev, int64_t n, int64_t T,
                               int staged, void* spot_dev, int64_t max_peaks, double* thresholds_out_dev,
                               const mtadgat_stream_outputs* out, void* stream);
/* mtadgat_stream_flush with reset for the selected streams, and their SPOT columns restored from a calibrated state of one
 * column or n_streams columns. */
int mtadgat_stream_reset_spot(mtadgat_handle h, void* state_dev, int64_t n_streams, int64_t max_block, void* spot_dev,
                              const void* spot_calibrated_dev, int64_t calibrated_columns, int64_t max_peaks,
                              const int64_t* streams_dev, int64_t n, void* stream);

/* ---- preparing raw series: scaler, gap fill, inverse, streams (csrc/mtadgat_prep.hip; preparation.py) ---------------------
 * The first step of the reference's pipeline (utils.normalize_data: NaN replaced, a MinMaxScaler fitted on the training series and
 * applied to train and test) for device-resident data, plus a causal fill for sensor drop-outs.  tests/prep_refs.py states the
 * definitions in numpy.  Conventions of the part calls above: handle-free, no atomics, no library kernels, bitwise reproducible,
 * status 0 / -1 / -3 / -5 with a mtadgat_last_error() message, every argument is checked before anything touches the device,
 * asynchronous on `stream`, nothing is read back.  Arrays are (n, d) float32 with a row stride ld >= d, 1 <= n <= 2^31 - 1,
 * 1 <= d <= 2048, ld < 2^31.  Scratch is 8-byte aligned, at least what the _scratch function returns (0 for refused sizes) and
 * need not be initialised.  Rows are reduced and scanned in fixed blocks of mtadgat_prep_rows_per_block() rows.
 *
 * A GAP is a sample that is not finite: NaN, +inf or -inf (the reference's nan_to_num would turn an infinity into +-3.4e38, which
 * no scaler survives).
 *
 * mtadgat_prep_fit: one record per column of x_dev into scaler_dev (d records on the device).  gaps = 0 (ignore) leaves the gaps
 * out, sklearn's own behaviour; gaps = 1 (zero) counts every gap as the sample 0.0, the reference's (nan_to_num runs before its
 * fit).  lo / hi: the exact minimum and maximum of the samples; n_valid their number; mean: their float64 sum -- per row block a
 * fixed tree, the blocks added in order -- divided once and rounded once to float32.  A column without a sample has lo = hi =
 * mean = 0.  In float32, every operation rounded on its own: range = hi - lo; scale = 1 / (range < 10 eps32 ? 1 : range);
 * offset = 0 - lo scale -- MinMaxScaler's scale_ and min_ bit for bit.
 *
 * mtadgat_prep_transform: out = fl(fl(v scale) + offset), clipped to [0, 1] when clip != 0, where v is x or, at a gap, by fill:
 * 0 (none) NaN; 1 (zero) the raw value 0.0; 2 (hold) the raw value of the last valid sample of the column within the row's part,
 * the column's mean when the part has none before the row.  The parts are `count` disjoint ascending row spans [start_k, end_k)
 * on the device (int64), as in the part calls above; every span start and every span end is a seam no fill looks across, so rows
 * that no span covers form stretches of their own; count = 0 (start_dev, end_dev may be NULL): one part.  age_dev (NULL, or (n, d)
 * int32, contiguous): 0 at a valid sample, k at the k-th consecutive gap row since the last valid one, counted from the part's
 * first row (i - part_start + 1) where the part has none yet.  fill 0 / 1 without age is one launch and needs no scratch; the hold
 * fill and the age are a blocked scan of three launches (csrc/mtadgat_prep.hip).  out_dev may be x_dev (with ld_out = ld) and
 * must not overlap it otherwise.
 *
 * mtadgat_prep_inverse: out[i, j] = fl(fl(y[i, j] - offset) / scale) with the record of column dims_dev[j] (int32 on the device;
 * NULL: column j, then d <= d_scaler) of a scaler of d_scaler columns; NaN where dims_dev[j] lies outside it.
 *
 * mtadgat_prep_stream_*: the same fill as per-stream state for rows that arrive a few at a time.  One allocation of
 * mtadgat_prep_stream_state_bytes() bytes (16-byte aligned) that the host never reads holds, per (stream, column), the last valid
 * raw value, whether there was one, and the age; _init writes it, _reset returns the selected streams (streams_dev NULL: 0 ..
 * n - 1) to "nothing heard yet".  _push: rows_dev (n, T, d) float32 for the n distinct streams streams_dev (int64 on the device;
 * NULL: 0 .. n - 1) in (stream, t) order; out_dev (n, T, d) and age_dev (NULL or (n, T, d) int32) are what mtadgat_prep_transform
 * gives for the stream's rows so far as one part, however they were cut into pushes.  A stream index outside [0, n_streams)
 * touches no state and gets NaN (age -1); so does every row when the state was initialised for other sizes. */
typedef struct mtadgat_prep_column {
    float   lo, hi, scale, offset, mean;
    int32_t n_valid;
} mtadgat_prep_column;
int mtadgat_prep_rows_per_block(void);
size_t mtadgat_prep_fit_scratch(int64_t n, int d);
int mtadgat_prep_fit(const float* x_dev, int64_t n, int d, int64_t ld, int gaps, void* scratch_dev, size_t scratch_bytes,
                     mtadgat_prep_column* scaler_dev, void* stream);
size_t mtadgat_prep_transform_scratch(int64_t n, int d, int fill, int want_age);
int mtadgat_prep_transform(const float* x_dev, int64_t n, int d, int64_t ld, const mtadgat_prep_column* scaler_dev, int fill, int clip,
                           const int64_t* start_dev, const int64_t* end_dev, int64_t count, void* scratch_dev, size_t scratch_bytes,
                           float* out_dev, int64_t ld_out, int32_t* age_dev, void* stream);
int mtadgat_prep_inverse(const float* y_dev, int64_t n, int d, int64_t ld, const mtadgat_prep_column* scaler_dev, int d_scaler,
                         const int32_t* dims_dev, float* out_dev, int64_t ld_out, void* stream);
size_t mtadgat_prep_stream_state_bytes(int64_t n_streams, int d);
int mtadgat_prep_stream_init(void* state_dev, int64_t n_streams, int d, void* stream);
int mtadgat_prep_stream_push(void* state_dev, int64_t n_streams, int d, const float* rows_dev, const int64_t* streams_dev, int64_t n,
                             int64_t T, const mtadgat_prep_column* scaler_dev, int fill, int clip, float* out_dev, int32_t* age_dev,
                             void* stream);
int mtadgat_prep_stream_reset(void* state_dev, int64_t n_streams, int d, const int64_t* streams_dev, int64_t n, void* stream);

/* Per-kernel launch timing for bench.py's roofline leg: when enabled, forward()
 * brackets each kernel family with hipEvents on `stream`; mtadgat_profile_read
 * synchronises those events and returns accumulated milliseconds + launch counts
 * since the last read.  names: "conv","proj","attend","gru","fc","recon". */
#define MTADGAT_PROFILE_SLOTS 6
int mtadgat_profile_enable(mtadgat_handle h, int on);
int mtadgat_profile_read(mtadgat_handle h, double ms[MTADGAT_PROFILE_SLOTS],
                         int64_t launches[MTADGAT_PROFILE_SLOTS]);
const char* mtadgat_profile_name(int slot);

#ifdef __cplusplus
}
#endif
#endif /* MTADGAT_H */
