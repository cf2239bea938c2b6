/*
 * arcle_hip.h — C ABI of the MI355X-native ARCLE hot path (libarcle_hip.so).
 *
 * This is the drop-in boundary for the reference's data-parallel hot path:
 *   O2ARCv2Env.step()/transition()      /root/reference/arcle/envs/o2arcenv.py:130-151
 *   ARCEnv.step()/transition()          /root/reference/arcle/envs/arcenv.py:155-176
 *   RawARCEnv.step()                    /root/reference/arcle/envs/arcenv.py:60-76
 *   AbstractARCEnv.submit()/init_state  /root/reference/arcle/envs/base.py:155-183
 *   the op closures of arcle/actions    color.py:62-103, object.py:10-349, critical.py:8-66
 *   BBoxWrapper/PointWrapper.action     /root/reference/arcle/wrappers/bbox.py:22-30,43-49
 *
 * The reference has no FFI of its own (it is pure Python); the functions below are what
 * a ctypes binding inside the reference's `step()` would call.
 *
 * Conventions
 *   - every pointer in `arcle_buffers` and every per-step array is a DEVICE pointer
 *     (HBM of the GPU the handle was created on); plain C types only, no torch types.
 *   - all functions return 0 on success or a negative arcle_status; they never throw.
 *   - kernels are enqueued on the `hipStream_t` passed as `void* stream` (NULL = default
 *     stream) and are asynchronous; outputs are valid after the stream is synchronised.
 *   - a handle is not thread-safe; serialise calls on one handle (the reference env is
 *     single-threaded as well).
 *
 * State layout in HBM (structure of arrays, all int8, one row per env):
 *   plane[p]  : int8 [n_envs][PS]    env e's H x W cells are the first H*W bytes (row-major: row, col) of row e; the
 *                                    row stride PS = arcle_config.plane_stride (default: H*W rounded up to 128 B,
 *                                    e.g. 1024 for 30x30); bytes [H*W, PS) of every row are zero padding.
 *                                    p in arcle_plane
 *   rec       : int8 [n_envs][16]    packed per-env scalars, byte offsets ARCLE_REC_*
 *   cnt       : int32[n_envs][2]     {action_steps, submit_count}
 */
#ifndef ARCLE_HIP_H
#define ARCLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARCLE_ABI_VERSION 18
#define ARCLE_MAX_OPS 64
#define ARCLE_MAX_CELLS 1024 /* H*W <= 1024: one 64-lane wavefront x 16 cells holds a plane (the one-wavefront-per-env kernels);
                                larger planes (H, W <= 127) are served by the workgroup-per-env kernels — see "Grids beyond
                                ARCLE_MAX_CELLS" below */
#define ARCLE_PLANE_SLACK 1024 /* readable bytes wanted BEHIND the answer plane's n_envs * plane_stride (the library's own planes all have
                                  them): arcle_transition_rows requests that plane from all 64 lanes, 1024 bytes from the env's plane on */
#define ARCLE_MAX_SIDE 127   /* H, W <= 127: grid dims are int8 in the record (and in the reference's state dict, base.py:162-166) */
/* default per-env plane stride: H*W rounded up to a whole number of 128-byte lines (30x30 -> 1024 B), so that no two
 * envs share a cache line of a plane and every plane store writes full lines */
#define ARCLE_DEFAULT_PLANE_STRIDE(P) (((P) + 127) & ~127)

/* ---- planes: keys of the reference state dict (o2arcenv.py:16-34, base.py:155-166) ---- */
enum arcle_plane {
  ARCLE_PL_INPUT = 0,      /* state['input']                                        */
  ARCLE_PL_GRID = 1,       /* state['grid']                                         */
  ARCLE_PL_SELECTED = 2,   /* state['selected']                    (O2ARCv2Env)     */
  ARCLE_PL_CLIP = 3,       /* state['clip']                        (O2ARCv2Env/ARCEnv) */
  ARCLE_PL_OBJECT = 4,     /* state['object_states']['object']     (O2ARCv2Env)     */
  ARCLE_PL_OBJECT_SEL = 5, /* state['object_states']['object_sel'] (O2ARCv2Env)     */
  ARCLE_PL_BACKGROUND = 6, /* state['object_states']['background'] (O2ARCv2Env)     */
  ARCLE_PL_ANSWER = 7,     /* env.answer zero-padded to HxW (info['answer'], base.py:150) */
  ARCLE_N_PLANES = 8
};

/* ---- per-env scalar record, byte offsets into rec[env][16] (all int8) ---- */
#define ARCLE_REC_INPUT_DIM 0   /* [2] state['input_dim']                     */
#define ARCLE_REC_GRID_DIM 2    /* [2] state['grid_dim']                      */
#define ARCLE_REC_CLIP_DIM 4    /* [2] state['clip_dim']                      */
#define ARCLE_REC_OBJECT_DIM 6  /* [2] object_states['object_dim']            */
#define ARCLE_REC_OBJECT_POS 8  /* [2] object_states['object_pos'] (signed)   */
#define ARCLE_REC_TRIALS 10     /* [1] state['trials_remain']                 */
#define ARCLE_REC_TERMINATED 11 /* [1] state['terminated']                    */
#define ARCLE_REC_ACTIVE 12     /* [1] object_states['active']                */
#define ARCLE_REC_PARITY 13     /* [1] object_states['rotation_parity']       */
#define ARCLE_REC_ANSWER_DIM 14 /* [2] env.answer.shape                       */
#define ARCLE_REC_BYTES 16

#define ARCLE_CNT_STEPS 0  /* env.action_steps == info['steps']          */
#define ARCLE_CNT_SUBMIT 1 /* env.submit_count == info['submit_count']   */

/* ---- op descriptors: one uint32 per slot of the env's operation table ----
 * desc = kind | (arg << 8) | (flags << 16).  The table is what
 * AbstractARCEnv.create_operations() returns (base.py:140-142); slot index == the
 * integer `action['operation']`. */
enum arcle_op_kind {
  ARCLE_OP_NONE = 0,             /* empty slot (never valid to execute)                     */
  ARCLE_OP_COLOR = 1,            /* gen_color(arg)        color.py:62-77                    */
  ARCLE_OP_FLOODFILL = 2,        /* gen_flood_fill(arg)   color.py:79-103 (+dfs :8-30)      */
  ARCLE_OP_MOVE = 3,             /* gen_move(arg) 0=U 1=D 2=R 3=L    object.py:218-243      */
  ARCLE_OP_ROTATE = 4,           /* gen_rotate(arg) k=1,2,3 (CCW)    object.py:167-216      */
  ARCLE_OP_FLIP = 5,             /* gen_flip(axis) 0=H 1=V 2=D0 3=D1 object.py:245-279      */
  ARCLE_OP_COPY = 6,             /* gen_copy(src) 0="I" 1="O"        object.py:281-314      */
  ARCLE_OP_PASTE = 7,            /* gen_paste(paste_blank=arg)       object.py:316-349      */
  ARCLE_OP_COPY_FROM_INPUT = 8,  /* copy_from_input       critical.py:19-29                 */
  ARCLE_OP_RESET_GRID = 9,       /* reset_grid            critical.py:8-17                  */
  ARCLE_OP_RESIZE_GRID = 10,     /* resize_grid           critical.py:31-46                 */
  ARCLE_OP_CROP_GRID = 11,       /* crop_grid             critical.py:48-66                 */
  ARCLE_OP_RESIZE_TO_ANSWER = 12,/* RawARCEnv resize_to_answer  arcenv.py:31-35             */
  ARCLE_OP_SUBMIT = 13,          /* AbstractARCEnv.submit base.py:172-183                   */
  ARCLE_OP_HOST = 14,            /* slot of an arbitrary host callable (base.py:140-142): a device no-op — the step is
                                    counted, the host layer applies the callable to the fetched state               */
  ARCLE_N_OP_KINDS = 15
};
#define ARCLE_OPF_RESET_SEL 1u /* wrapped by reset_sel  object.py:10-26 */
#define ARCLE_OPF_KEEP_SEL 2u  /* wrapped by keep_sel   object.py:28-41 */
#define ARCLE_OP_DESC(kind, arg, flags) \
  ((uint32_t)(kind) | ((uint32_t)(arg) << 8) | ((uint32_t)(flags) << 16))
#define ARCLE_OP_KIND(d) ((d) & 0xffu)
#define ARCLE_OP_ARG(d) (((d) >> 8) & 0xffu)
#define ARCLE_OP_FLAGS(d) (((d) >> 16) & 0xffu)

/* ---- step flags ---- */
/* Envs whose `terminated` is already 1 when the step starts are re-initialised from their
 * task (init_state, base.py:155-166 + o2arcenv.py:16-34) instead of executing the action;
 * reward 0, terminated 0 for that step (Gymnasium "next-step" autoreset; not in the
 * reference, which keeps mutating a terminated env — that is the default here too). */
#define ARCLE_STEP_AUTORESET 1u
/* reset_sel (object.py:20-25) need not rewrite a `selected` plane that is already zero.  Whenever the op table holds
 * no keep_sel-wrapped op, `active == 0` implies `selected == 0` (object ops set both, reset_sel / init_state clear both,
 * nothing else writes `selected`), so with this flag the zero-fill is skipped when the env enters the step with
 * active == 0, and an object op that lifts a fresh selection in such an env stores `selected` only in the 16-byte chunks
 * the placed object covers (the rest is zero already).  The state after the step is bit-identical; only redundant writes
 * disappear.  Do NOT set it
 * for states written from outside (e.g. a state dict uploaded for transition()) that may violate the invariant;
 * arcle_set_op_table() reports through arcle_can_elide_selected() whether the installed table permits it. */
#define ARCLE_STEP_ELIDE_SELECTED 2u
/* also writes truncated[env] = (action_steps >= step_limit) into the array installed with arcle_set_truncation
 * (gymnasium TimeLimit(max_episode_steps) as the reference's training script applies it, agents/train.py:67) */
#define ARCLE_STEP_TRUNCATE 4u
/* like ARCLE_STEP_AUTORESET, but the env starts its next episode on a NEW task drawn on the device from the task table
 * (arcle_set_task_table + arcle_set_sampler): problem and pair uniform, optional colour-permutation / rot90
 * augmentation (agents/env.py:31-42), all keyed by (seed, global env id, episode number) */
#define ARCLE_STEP_RESAMPLE 8u
/* also writes dense[env] = (cells of grid that match the answer inside the common rectangle, total cells as in
 * agents/env.py:44-58) into the int32 [n_envs][2] array installed with arcle_set_dense_output: the research env's dense
 * reward is  sparse*100 - 1 + dense[0]/dense[1]  (formed by the host, exact integers on the device) */
#define ARCLE_STEP_DENSE 16u
/* mask ingress only: an object op (Move/Rotate/Flip) whose selection equals the env's current `selected` plane is
 * executed with an empty selection, i.e. continues the active object — the rule of the reference's O2ARC trace harness
 * (tests/o2arc_check.py:169-170) */
#define ARCLE_STEP_CONTINUE_RULE 32u
/* reset(options={'reset_on_submit': True}) (base.py:87-93,179-180): a Submit with trials left
 * re-initialises the env from its input inside the op; the caller sees the fresh state, terminated stays 0 */
#define ARCLE_STEP_RESET_ON_SUBMIT 64u
/* the step flags served by the feature instantiations of the step kernel (the plain ones stay lean) */
/* the step kernel also writes the flattened observation row (arcle_set_flat_output: FlattenObservation, optionally after
 * FilterO2ARC) of the state it produced — fused into the same launch */
#define ARCLE_STEP_FLAT_OBS 128u
/* the step kernel also writes the env's packed per-step row  grid | grid_dim | reward | terminated  (arcle_set_packed_output; the
 * record a central learner gathers from every GPU) — fused into the same launch */
#define ARCLE_STEP_PACK_OBS 256u
/* with ARCLE_STEP_FLAT_OBS: the row buffer still holds every env's row of the PREVIOUS step (same buffer, installed once, every
 * step of this handle run with ARCLE_STEP_FLAT_OBS since the rows were last written in full — by arcle_flatten_obs into that buffer or
 * by a step without this flag).  The writer then rewrites only the scalars and the segments of the planes this step stored; an
 * op touches one to five of the seven planes, so most of a row is left as it is.  The rows are byte-identical to full rewrites. */
#define ARCLE_STEP_ROWS_INCREMENTAL 512u
#define ARCLE_STEP_FEATURE_FLAGS                                                                                        \
  (ARCLE_STEP_RESAMPLE | ARCLE_STEP_DENSE | ARCLE_STEP_CONTINUE_RULE | ARCLE_STEP_RESET_ON_SUBMIT | ARCLE_STEP_FLAT_OBS | \
   ARCLE_STEP_PACK_OBS | ARCLE_STEP_ROWS_INCREMENTAL)

/* ---- augmentation of a task at reset (arcle_set_sampler / ARCLE_STEP_RESAMPLE / arcle_reset_sampled) ---- */
#define ARCLE_AUG_PERMUTE 1u /* random permutation of the colours 0..9 (applied to input and answer) */
#define ARCLE_AUG_ROT90 2u   /* np.rot90(., k) with k uniform in 0..3                                 */

/* ---- sticky device status bits (arcle_get_status) ---- */
#define ARCLE_ST_BAD_OP 1u       /* operation index out of range / empty slot: step skipped
                                    (reference: IndexError / TypeError)                   */
#define ARCLE_ST_BAD_TASK 4u      /* arcle_reset_from_table: task index outside the table: env left untouched */
#define ARCLE_ST_BAD_SELECTION 8u /* a point outside the H x W plane or a negative bbox / point coordinate: the reference
                                    raises IndexError (or NumPy wraps the negative index); here the selection is
                                    empty, the step runs, and this bit reports it                          */
#define ARCLE_ST_ROTATE_DOMAIN 2u /* Rotate produced a position outside int8 or a tile that
                                    does not fit HxW (reference: ValueError/garbage,
                                    SURVEY.md A.6-2, A.6-6): step skipped                  */

#define ARCLE_ST_AUG_DOMAIN 16u   /* arcle_reset_from_table_aug: an explicit rot90 by an odd count does not fit a non-square
                                    H x W plane: env left untouched (device-drawn augmentations drop the quarter turn instead) */

enum arcle_status {
  ARCLE_OK = 0,
  ARCLE_ERR_ARG = -1,     /* NULL / out-of-range argument                                */
  ARCLE_ERR_CONFIG = -2,  /* unsupported H, W, n_ops or op table needing absent planes   */
  ARCLE_ERR_HIP = -3,     /* a HIP runtime call failed; see arcle_last_error()           */
  ARCLE_ERR_NO_DEVICE = -4
};

typedef struct arcle_config {
  int32_t n_envs;    /* envs owned by this handle (this GPU's shard)                     */
  int32_t H, W;      /* max_grid_size (base.py:49); H, W <= ARCLE_MAX_SIDE (any such size: see "Grids beyond ARCLE_MAX_CELLS") */
  int32_t max_trial; /* base.py:51; stored as int8 in trials_remain                      */
  int32_t device;    /* HIP device ordinal, -1 = current device                          */
  int32_t plane_stride; /* bytes between consecutive envs of a plane (PS): 0 = default (ARCLE_DEFAULT_PLANE_STRIDE(H*W));
                           otherwise a multiple of 16 with H*W <= PS <= 1024 (<= 16256 for grids beyond ARCLE_MAX_CELLS) */
} arcle_config;

typedef struct arcle_buffers {
  int8_t* plane[ARCLE_N_PLANES]; /* NULL for planes the env kind does not have           */
  int8_t* rec;                   /* [n_envs][16]                                         */
  int32_t* cnt;                  /* [n_envs][2]                                          */
} arcle_buffers;

typedef struct arcle_env arcle_env; /* opaque handle */

/* ---- Grids beyond ARCLE_MAX_CELLS -----------------------------------------------------------------------------------------------
 * The reference takes any max_grid_size (base.py:37-49).  A handle with H * W <= ARCLE_MAX_CELLS runs the one-wavefront-per-env kernels
 * (ARC's own regime, 30 x 30: everything in this header applies).  A handle with H * W > ARCLE_MAX_CELLS (H, W <= ARCLE_MAX_SIDE) runs one
 * WORKGROUP per env (arcle_amd/csrc/arcle_big.hip): same layout (PS = H*W rounded up to 128), same entry points, same results bit for
 * bit against the reference's algorithm — with these differences:
 *   served      arcle_reset / _reset_from_table(_aug) / _reset_sampled (task augmentation included), arcle_step_mask / _bbox / _point / _bbox5 /
 *               _bits (+ arcle_pack_mask_bits; rows of plane_stride / 8 bytes), arcle_step_many, arcle_rollout_*
 *               (= n_steps step launches: the state does not fit a wavefront's registers), arcle_transition_rows (three launches over
 *               library-owned scratch envs, allocated on first use: not inside a stream capture), arcle_flatten_obs / _get_state_rows /
 *               _set_state_rows, arcle_pack_obs, planes, status; step flags AUTORESET, ELIDE_SELECTED, TRUNCATE, RESAMPLE, DENSE (the pair is
 *               computed from the planes every step: no cache), CONTINUE_RULE, RESET_ON_SUBMIT, FLAT_OBS (tail and completion signal
 *               included), PACK_OBS; ROWS_INCREMENTAL is accepted and rewrites the rows in full (identical bytes)
 *   accounting  arcle_enable_accounting counts every 16-byte access the threads issue (planes, table entries, mask chunks, rows in) + the
 *               env's scalars as `issued`; the `bytes` figure is the same without the row padding (x H*W / plane_stride)
 *   no-ops      arcle_set_dispatch_order, arcle_hint_next_ops, arcle_autotune (returns 0 candidates: one launch plan), arcle_launch_info
 *               reports {0, 0, waves per workgroup, 0}
 * Action arrays and row buffers may be device or pinned host memory as everywhere else. */

/* Creates a handle. `bufs` are caller-owned device buffers (e.g. torch tensors' data_ptr);
 * if bufs == NULL the library allocates all planes itself (hipMalloc) and frees them in
 * arcle_destroy. Replaces AbstractARCEnv.__init__ state allocation (base.py:37-66).
 * A caller-owned answer plane with plane_stride < 1024 must be followed by ARCLE_PLANE_SLACK - plane_stride readable bytes (any
 * content, never written): arcle_transition_rows reads 1024 bytes from the env's plane on whatever the stride, so for the handle's
 * last envs it reads behind the plane (arcle_amd.engine.EnvBatch allocates every plane with that slack). */
int arcle_create(const arcle_config* cfg, const arcle_buffers* bufs, arcle_env** out);
int arcle_destroy(arcle_env* env);
/* Fills `out` with the device pointers the handle uses. */
int arcle_get_buffers(const arcle_env* env, arcle_buffers* out);

/* Installs the operation table (host array of descriptors). Replaces the list returned by
 * create_operations() (o2arcenv.py:76-113, arcenv.py:26-41,110-138). */
int arcle_set_op_table(arcle_env* env, const uint32_t* descs, int32_t n_ops);

/* 1 if the installed op table keeps the invariant documented at ARCLE_STEP_ELIDE_SELECTED, else 0. */
int arcle_can_elide_selected(const arcle_env* env);

/* Re-initialises envs from PL_INPUT / REC_INPUT_DIM (init_state: base.py:155-166,
 * o2arcenv.py:16-34; counters as in reset base.py:73-79). `mask` is a device uint8[n_envs]
 * (non-zero = reset) or NULL for all envs. The task (input, answer, dims) must have been
 * written into PL_INPUT, PL_ANSWER, REC_INPUT_DIM, REC_ANSWER_DIM by the host layer. */
int arcle_reset(arcle_env* env, const uint8_t* mask, void* stream);

/* Device task table: n_tasks (input, answer) pairs, already zero-padded to the plane stride PS = H*W rounded up
 * (arcle_config.plane_stride): in_planes / ans_planes int8 [n_tasks][PS], in_dims / ans_dims int8 [n_tasks][2] (device pointers, owned
 * by the caller, must stay alive).  It is the packed form of what Loader.parse yields (loader.py:89-113), one entry
 * per (task, pair).  Alignment (ABI 5): the planes 16 bytes; the dims arrays 4 bytes, their allocation covering 2 * n_tasks rounded up
 * to a multiple of 4 bytes (an entry's two dims are read with one aligned dword load) — misaligned arrays are rejected. */
int arcle_set_task_table(arcle_env* env, const int8_t* in_planes, const int8_t* in_dims, const int8_t* ans_planes,
                         const int8_t* ans_dims, int32_t n_tasks);
/* reset() with the task choice made by the caller (base.py:95-108): for every env with mask[env] != 0 (mask NULL =
 * all) copies table entry task_idx[env] (device int32[n_envs]) into PL_INPUT / PL_ANSWER / REC_*_DIM and runs
 * init_state.  No host loop, no host->device copy of grids. */
int arcle_reset_from_table(arcle_env* env, const int32_t* task_idx, const uint8_t* mask, void* stream);

/* One step() of every env. Replaces O2ARCv2Env.step (o2arcenv.py:130-147).
 *   op      device int32[n_envs]       action['operation']
 *   reward  device int32[n_envs] out   0/1 (o2arcenv.py:121-128)
 *   term    device uint8[n_envs] out   bool(state['terminated'][0])
 * selection ingress, three forms:
 *   _mask : sel  device int8 [n_envs][H*W]   action['selection'] as given
 *   _bbox : bbox device int32[n_envs][4]     (x1,y1,x2,y2) as BBoxWrapper.action (bbox.py:22-30)
 *   _point: xy   device int32[n_envs][2]     (x,y)         as PointWrapper.action (bbox.py:43-49)
 */
int arcle_step_mask(arcle_env* env, const int8_t* sel, const int32_t* op, int32_t* reward,
                    uint8_t* term, uint32_t flags, void* stream);
int arcle_step_bbox(arcle_env* env, const int32_t* bbox, const int32_t* op, int32_t* reward,
                    uint8_t* term, uint32_t flags, void* stream);
int arcle_step_point(arcle_env* env, const int32_t* xy, const int32_t* op, int32_t* reward,
                     uint8_t* term, uint32_t flags, void* stream);

/* Two more forms of the action, same step():
 *   _bbox5: act5 device int32[n_envs][5]   the BBoxWrapper action as ONE record per env (x1, y1, x2, y2, operation) — exactly the
 *           5-tuple `BBoxWrapper.action` receives (bbox.py:22-30, examples/example_bbox.py:13-15); no separate op array, so a
 *           host-resident policy moves its actions with one 20-byte-per-env copy (or none: act5 may be pinned host memory)
 *   _bits : bits device uint8[n_envs][128] boolean selection masks, bit-packed: bit (f & 7) of byte (f >> 3) of row e = cell f
 *           (row-major, f = row * W + col) of env e is selected; rows are ARCLE_MAX_CELLS / 8 = 128 bytes apart (handles of more than
 *           ARCLE_MAX_CELLS cells: plane_stride / 8 bytes — arcle_mask_bits_stride() says which), 2-byte aligned.
 *           `create_action_space` accepts boolean masks (base.py:134-138); packed they are 1/8 of the int8 traffic and need no
 *           byte -> bit reduction in the kernel.  arcle_pack_mask_bits converts int8 [n_envs][H*W] masks (truthy = non-zero). */
enum arcle_ingress { ARCLE_INGRESS_MASK = 0, ARCLE_INGRESS_BBOX = 1, ARCLE_INGRESS_POINT = 2, ARCLE_INGRESS_BBOX5 = 3, ARCLE_INGRESS_BITS = 4 };
int arcle_step_bbox5(arcle_env* env, const int32_t* act5, int32_t* reward, uint8_t* term, uint32_t flags, void* stream);
int arcle_step_bits(arcle_env* env, const uint8_t* bits, const int32_t* op, int32_t* reward, uint8_t* term, uint32_t flags,
                    void* stream);
int arcle_pack_mask_bits(arcle_env* env, const int8_t* sel, uint8_t* bits, void* stream);
int arcle_mask_bits_stride(const arcle_env* env); /* bytes between the envs' rows of a bit-packed mask array */

/* n_steps consecutive step() LAUNCHES enqueued by ONE call (the loop `for t in range(n): env.step(actions[t])` of a caller that
 * holds the actions of the next n steps; every step is a full step(): state observable in between on the stream, all step flags
 * valid).  `ingress`: arcle_ingress; sel: the form's payload [n_steps][n_envs][...]; op int32 [n_steps][n_envs] (NULL for BBOX5);
 * reward int32 [n_steps][n_envs], term uint8 [n_steps][n_envs] out.  Per-handle outputs (truncated, dense, flat / packed rows) hold
 * the LAST step's values afterwards.  Capturable into a hipGraph like the single-step calls (no synchronisation).
 * Host-resident actions: with ARCLE_INGRESS_BBOX5 `sel` may be PINNED HOST memory (the records of a policy that runs on the CPU).
 * For the standard 30 x 30 batch stepped with ARCLE_STEP_AUTORESET | ARCLE_STEP_ELIDE_SELECTED the library then pipelines the PCIe
 * traffic: eight extra workgroups at the front of launch t copy step t+1's records into a device staging buffer while launch t
 * runs, and step t+1 reads them from HBM (only step 0 reads across PCIe itself).  The staging buffer (2 x 20 B per env) is allocated
 * by the first such call made outside a stream capture. */
int arcle_step_many(arcle_env* env, int ingress, int32_t n_steps, const void* sel, const int32_t* op, int32_t* reward,
                    uint8_t* term, uint32_t flags, void* stream);
/* Dispatch order (ABI 5).  A launch of one wave per env ends with its last Move / Rotate / Flip wave (they run ~1.2 us longer than the
 * other operations' waves, and the hardware starts the waves of a launch over ~2 us), so the library hands the object operations to
 * the waves that start first.  Since ABI 5 every launch does that for ITSELF, from the operations it is about to execute: the standard
 * 30 x 30 batch (plane stride 1024) stepped through arcle_step_bbox / _bbox5 / _point / _mask / _bits — and arcle_step_many over them — with
 * the flag set ARCLE_STEP_AUTORESET | ARCLE_STEP_ELIDE_SELECTED; the tuple forms also with ARCLE_STEP_ELIDE_SELECTED alone (no auto-reset);
 * bbox / bbox5 also with ARCLE_STEP_AUTORESET | _ELIDE_SELECTED | _PACK_OBS or the research env's set with incremental FilterO2ARC rows; n_envs a multiple of 256 in [2304, 10240], actions in DEVICE memory, an op table with object operations, no byte
 * accounting.  Waves of a group of 32 consecutive envs read the group's 32 actions and permute the group among their 32 dispatch slots
 * (arcle_step_kernel, GROUPED; arcle_group.h).  The permutation is computed from launch-constant inputs only (the group's operation indices
 * and the op table: nothing a wave of the launch writes), so the 32 waves agree on it whenever each of them starts.  Scheduling only: every
 * env is stepped exactly once whatever the operations are; results, outputs and their layout are those of the plain launch.  No tables, no extra memory, nothing to allocate before a stream capture.
 * arcle_set_dispatch_order(env, 0) turns it off for the handle (default on).
 * arcle_hint_next_ops: ABI 4's one-shot hint of the NEXT step's operations (the table form of ordered dispatch needed them a step
 * ahead).  Still accepted and validated — stride 1 for op arrays, 5 for the op field of BBoxWrapper records — and ignored. */
int arcle_set_dispatch_order(arcle_env* env, int enable);
int arcle_hint_next_ops(arcle_env* env, const int32_t* next_op, int32_t stride);
/* How a step launch of this handle runs, chosen by batch size from tables measured on one MI355X with a cache-resident action stream:
 * the cache policy of the speculative grid request (0 none; 'A' spec + write-through stores, small batches; 'B' + non-temporal stores,
 * 'H' non-temporal request, 'J' both: state beyond the 256 MiB Infinity Cache), the workgroup size (4 or 8 waves), and whether the
 * launch orders itself.  arcle_launch_info reports the plan a launch with (ingress, flags) and device-resident actions would take:
 * out4 = {orders itself, policy (0 or the letter), waves per workgroup, 1 if arcle_autotune chose it}.
 * arcle_autotune replaces the tables for THIS handle: it times every plan the launch can take — on this handle's batch size, this box and
 * the caller's own action arrays where they live (n_batches consecutive action batches laid out as for arcle_step_many: sel
 * [n_batches][n_envs][...], op [n_batches][n_envs]; a representative stretch of the policy's output — ONE repeated batch is not: the
 * state degenerates under it; ingress BBOX, BBOX5, POINT, MASK or BITS; flags within ARCLE_STEP_AUTORESET | _ELIDE_SELECTED | _PACK_OBS)
 * — 48 .. 96 warm-up launches (the caches' steady state: fewer mis-rank the non-temporal policies) and 24 .. 64 timed ones each, walking
 * the batches in order — and keeps the fastest for later launches with the same ingress and flags.  The env state is saved first and restored before every candidate and at the end (a temporary copy of the state
 * in device memory; reward / terminated of the timed launches go to scratch): the handle is left exactly as it was found.  Synchronises
 * the stream; not inside a stream capture.  report (may be NULL): int32 [report_rows][4] = {orders itself, policy, waves per workgroup,
 * ns per launch} per candidate timed.  Returns the number of candidates timed (>= 0) or a negative ARCLE_ERR_* code. */
int arcle_launch_info(arcle_env* env, int ingress, uint32_t flags, int32_t* out4);
int arcle_autotune(arcle_env* env, int ingress, int32_t n_batches, const void* sel, const int32_t* op, uint32_t flags, int32_t* report,
                   int32_t report_rows, void* stream);

/* n_steps consecutive step()s of every env in ONE launch — a rollout / trace replay for callers that already hold
 * the whole action sequence (the loop `for a in trace: env.step(a)`, e.g. tests/o2arc_check.py:139-199 of the
 * reference).  Semantically identical to n_steps calls of arcle_step_bbox/_point; the env state is kept on chip
 * between the steps, so only the final state is observable afterwards.
 *   bbox / xy  device int32[n_steps][n_envs][4 | 2]      op      device int32[n_steps][n_envs]
 *   reward     device int32[n_steps][n_envs] out         term    device uint8[n_steps][n_envs] out
 * flags: ARCLE_STEP_AUTORESET | _ELIDE_SELECTED; mask ingress also _CONTINUE_RULE | _RESET_ON_SUBMIT; and (ABI 5) ARCLE_STEP_PACK_OBS:
 * the launch then also writes the packed observation row of EVERY step — the buffer installed with arcle_set_packed_output must hold
 * uint8 [n_steps][n_envs][arcle_packed_obs_size()] — so an action-chunk caller keeps Gym's "observation after every step". */
int arcle_rollout_bbox(arcle_env* env, int32_t n_steps, const int32_t* bbox, const int32_t* op, int32_t* reward,
                       uint8_t* term, uint32_t flags, void* stream);
int arcle_rollout_point(arcle_env* env, int32_t n_steps, const int32_t* xy, const int32_t* op, int32_t* reward,
                        uint8_t* term, uint32_t flags, void* stream);
/* the same with full selection masks: sel device int8 [n_steps][n_envs][H*W] (the O2ARC trace replayer's form,
 * tests/o2arc_check.py:139-199 of the reference) */
int arcle_rollout_mask(arcle_env* env, int32_t n_steps, const int8_t* sel, const int32_t* op, int32_t* reward,
                       uint8_t* term, uint32_t flags, void* stream);

/* (ABI 6) The same rollout with the research env's step flags and EVERY step's outputs: identical to n_steps calls of arcle_step_*
 * with the same flags, the rows written in full.  ingress ARCLE_INGRESS_BBOX | _POINT | _MASK (sel as above).
 * flags: everything a step accepts except ARCLE_STEP_ROWS_INCREMENTAL (the mask-only rules of CONTINUE_RULE / RESET_ON_SUBMIT hold);
 * TRUNCATE takes the step limit installed with arcle_set_truncation (positive), RESAMPLE the sampler of arcle_set_sampler.  Step t writes
 * slice t of every output of `out`, device arrays the caller owns (the arrays installed with the setters are not written):
 *   trunc   uint8 [n_steps][n_envs]                                           (ARCLE_STEP_TRUNCATE)
 *   dense   int32 [n_steps][n_envs][2]                                        (ARCLE_STEP_DENSE)
 *   rows    int8  [n_steps][n_envs][rows_stride], rows_stride = arcle_flat_obs_size(env, rows_filtered) rounded up to 16, 16-byte
 *           aligned, no tail                                                  (ARCLE_STEP_FLAT_OBS)
 *   packed  uint8 [n_steps][n_envs][arcle_packed_obs_size()], 16-byte aligned (ARCLE_STEP_PACK_OBS)
 * An env may end several episodes inside one launch; episode / cur_task of the sampler describe the state after the last step.  The
 * dense-pair cache is dropped (as by every rollout).  A missing output, a wrong stride, TRUNCATE without a positive step limit, RESAMPLE
 * without a sampler or ROWS_INCREMENTAL is refused (ARCLE_ERR_ARG / _CONFIG) before anything is enqueued. */
typedef struct {
  uint8_t* trunc;
  int32_t* dense;
  int8_t* rows;
  int32_t rows_stride;
  int32_t rows_filtered;
  uint8_t* packed;
} arcle_rollout_out;
int arcle_rollout_ex(arcle_env* env, int ingress, int32_t n_steps, const void* sel, const int32_t* op, int32_t* reward, uint8_t* term,
                     const arcle_rollout_out* out, uint32_t flags, void* stream);

/* Device-side task choice.  pair_off / pair_cnt: device int32 [n_problems] — first task-table entry and number of
 * entries (pairs) of every problem that has at least one (Loader.pick's candidates for the current adaptation mode);
 * episode: device int32 [n_envs] episodes started so far (the RNG stream position; the library increments it);
 * cur_task: device int32 [n_envs] or NULL, receives the table index each env currently runs; env_base: global id of
 * this handle's env 0 (multi-GPU shards), aug_flags: ARCLE_AUG_*.  The draw is a pure function of
 * (seed, env_base + env, episode[env]) — see arcle::draw_task. */
int arcle_set_sampler(arcle_env* env, const int32_t* pair_off, const int32_t* pair_cnt, int32_t n_problems, uint64_t seed,
                      int64_t env_base, int32_t* episode, int32_t* cur_task, uint32_t aug_flags);
/* reset() of the masked envs (mask NULL = all) onto device-drawn tasks (arcle_set_sampler). */
int arcle_reset_sampled(arcle_env* env, const uint8_t* mask, void* stream);
/* arcle_reset_from_table with an explicit augmentation per env: aug_k device uint8 [n_envs] (np.rot90 count) and/or
 * aug_perm device uint8 [n_envs][16] (perm[c] for colour c < 10); NULL = none. */
int arcle_reset_from_table_aug(arcle_env* env, const int32_t* task_idx, const uint8_t* mask, const uint8_t* aug_k,
                               const uint8_t* aug_perm, void* stream);
/* Installs the output of ARCLE_STEP_DENSE: dense_out device int32 [n_envs][2]; NULL removes it.  (0, 0) is written for a step that
 * executed no action (the auto-reset step of an env, a skipped step): "no dense term".  The library keeps the pair of every env's
 * current grid in a cache of its own and recomputes it only when a step stored the grid plane; a step or rollout launched WITHOUT
 * ARCLE_STEP_DENSE on such a handle drops the whole cache first (stream-ordered), so the pairs never describe a grid that moved. */
int arcle_set_dense_output(arcle_env* env, int32_t* dense_out);
/* For code that edits state planes BEHIND the library's back (plain copies into the buffers of arcle_get_buffers, host-applied
 * op slots): forget everything derived from the state (the dense-pair cache).  The library's own writers (reset kernels,
 * arcle_set_state_rows, auto-reset) do this themselves.  Asynchronous on `stream`. */
int arcle_invalidate(arcle_env* env, void* stream);

/* Installs the output of ARCLE_STEP_TRUNCATE: trunc_out device uint8[n_envs], step_limit = max_episode_steps.
 * trunc_out == NULL removes it. */
int arcle_set_truncation(arcle_env* env, uint8_t* trunc_out, int32_t step_limit);

/* Flattened observation — what the reference's policies consume.  One row per env holding the state dict in Gymnasium
 * FlattenObservation order (keys sorted, nested object_states in place; agents/models/GPTPolicy.py:17-35
 * `unflatten_vec`):  clip, clip_dim, grid, grid_dim, input, input_dim, active, background, object, object_dim,
 * object_pos, object_sel, rotation_parity, selected, terminated, trials_remain = 7*H*W + 14 bytes for O2ARCv2Env (6314 at
 * 30x30; env kinds without some keys omit them), or — filtered != 0 — the FilterO2ARC subset the reference's training
 * script flattens (agents/env.py:109-126, agents/train.py:61-68): active, clip, clip_dim, grid, grid_dim, object,
 * object_dim, object_pos, trials_remain = 3*H*W + 10 bytes (2710).
 * arcle_flat_obs_size() is that logical row length; `out` is a device buffer int8 [n_envs][out_stride], 16-byte aligned,
 * out_stride a multiple of 16 >= the length (the tail of every row is zero).  Rows are written with aligned, fully
 * coalesced 16-byte stores. */
int arcle_flat_obs_size(const arcle_env* env, int filtered);
int arcle_flatten_obs(arcle_env* env, int8_t* out, int32_t out_stride, int filtered, void* stream);
/* Destination of ARCLE_STEP_FLAT_OBS: every step call carrying that flag also writes the observation rows of the state it
 * produced (same stream, one ABI call per step, no host round trip).  out == NULL removes it. */
int arcle_set_flat_output(arcle_env* env, int8_t* out, int32_t out_stride, int filtered);

/* The same with tail != 0: the LAST 16 bytes of every row's stride then carry the step outputs of the env —
 *   int32 reward | int32 action_steps | int32 submit_count | uint8 terminated | uint8 truncated | uint8 status | 0
 * (status: the ARCLE_ST_* bits THIS env raised in THIS step) — so that one copy of the row (or none, when `out` is pinned host
 * memory) returns everything step() returns.  out_stride >= arcle_flat_obs_size() rounded up to 16, plus 16. */
int arcle_set_flat_output_ex(arcle_env* env, int8_t* out, int32_t out_stride, int filtered, int tail);
/* Completion signal in the row tail (ABI 5): with seq in 1..255 the LAST byte of every tail written from now on — by steps carrying
 * ARCLE_STEP_FLAT_OBS and by arcle_transition_rows with a tail — holds `seq`, and that word is stored last, behind a release at
 * system scope: a host that finds `seq` in the tail of a row in PINNED memory also finds the whole row and the other tail words.  It
 * can therefore poll that byte instead of synchronising the stream (a blocking synchronise wakes up tens of microseconds late): what
 * the single-env classes do — the caller changes seq from launch to launch.  0 (default) writes the tail as one plain 16-byte store. */
int arcle_set_flat_seq(arcle_env* env, int32_t seq);

/* ---- state rows at the boundary -------------------------------------------------------------------------------------------
 * A "state row" is the full (unfiltered) flattened observation of one env: the reference's state dict (base.py:155-166,
 * o2arcenv.py:16-34) as arcle_flat_obs_size(env, 0) bytes in FlattenObservation order.
 *   arcle_get_state_rows   = arcle_flatten_obs(.., filtered = 0): resident state -> rows (16-byte aligned, stride multiple of 16)
 *   arcle_set_state_rows   rows -> resident state of env e for every e with mask[e] != 0 (mask NULL = all); any row alignment /
 *                          stride >= the row length.  The inverse of the above: get + set is a checkpoint / restore of the state
 *                          dict (the task side — answer, answer_dim — and the counters are not part of a row and stay).
 *   arcle_transition_rows  the reference's `transition(state, action)` (o2arcenv.py:149-151; README.md:55
 *                          `env.transition(deepcopy(state), action)`) for a BATCH of (state, action) pairs: row r of rows_in + action r
 *                          -> row r of rows_out; the handle's resident envs are not touched, so any number of hypothetical states
 *                          (planning / search) can be expanded per launch.  Submit and the reward compare with the answer of resident
 *                          env src_env[r] (device int32[n_rows]; NULL = env r, then n_rows <= n_envs).  ingress: ARCLE_INGRESS_MASK /
 *                          _BBOX / _POINT / _BITS with the matching `sel` array [n_rows][...] (_BITS: uint8 [n_rows][128] as for
 *                          arcle_step_bits, 2-byte aligned; handles of at most ARCLE_MAX_CELLS cells per plane only — on a larger
 *                          grid the form is refused with ARCLE_ERR_ARG before any allocation or launch); op int32[n_rows]; reward int32[n_rows],
 *                          term uint8[n_rows] out; tail as arcle_set_flat_output_ex (action_steps = 1, submit_count = 1 iff the
 *                          Submit counted, base.py:174-175).  flags: ARCLE_STEP_RESET_ON_SUBMIT | _DENSE | _CONTINUE_RULE
 *                          (the rule compares cells: _MASK or _BITS selections, ARCLE_ERR_CONFIG with tuples).
 *                          rows_out may equal rows_in when the strides agree: IN PLACE, only the planes the op changed (and the scalars)
 *                          are rewritten — about half the time of the out-of-place form. */
int arcle_get_state_rows(arcle_env* env, int8_t* rows, int32_t stride, void* stream);
int arcle_set_state_rows(arcle_env* env, const int8_t* rows, int32_t stride, const uint8_t* mask, void* stream);
int arcle_transition_rows(arcle_env* env, int32_t n_rows, const int8_t* rows_in, int32_t in_stride, int ingress, const void* sel,
                          const int32_t* op, const int32_t* src_env, int8_t* rows_out, int32_t out_stride, int tail,
                          int32_t* reward, uint8_t* term, uint32_t flags, void* stream);
/* ---- search on state rows: a state hash, and K candidate actions per row ----------------------------------------------------------
 * hash [r][2] = (state_hash, grid_hash) of state row r.  state_hash is a function of the CONTENT of the row alone (every plane and
 * scalar field the env kind's row carries; not of its address, alignment, stride, padding, env or answer); grid_hash covers `grid`
 * and `grid_dim` only.  The formula (uint32 arithmetic, wrapping), with the finalisers
 *     fa(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
 *     fb(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * and a term pair  T(d, t) = (fa(d ^ (t * 0x9E3779B1)), fb(d + t * 0x85EBCA77))  of a dword d under the tag t:
 *     plane term(pl)  = sum over j < ceil(H*W / 4) of T(little-endian dword j of the plane's H*W bytes, zero-extended; (pl + 1) * 256 + j)
 *     record term     = sum over i < 4 of T(dword i of the 16-byte record with every byte the row does not carry — answer_dim, and
 *                       the fields the env kind lacks — set to zero; 0x0F00 + i)
 *     (A, B)          = sum of the terms of every plane of the row (pl = enum arcle_plane) + the record term
 *     state_hash      = A | B << 32
 *     grid_hash       = the same from plane term(ARCLE_PL_GRID) + T(record dword 0 with the input_dim bytes zeroed, 0x0E00)
 * Each (dword, plane, position) passes a nonlinear finaliser before the sum, so equal changes at two positions do not cancel; the sum
 * makes the hash decomposable by plane (a child's hash = the parent's with the terms of the changed planes and the record replaced).
 * arcle_amd/search.py::hash_rows_numpy is the same formula in NumPy.  One wavefront per row, any row alignment, stride >= the row length.
 *
 * arcle_expand_rows: K = n_actions candidate actions per state row, nothing but verdicts written.  rows [n_rows] are read only.
 * Actions: ARCLE_INGRESS_BBOX (sel int32 [..][4]), ARCLE_INGRESS_POINT (int32 [..][2]) or ARCLE_INGRESS_BITS (uint8 [..][S], S =
 * arcle_mask_bits_stride(): bit-packed boolean masks in the layout of arcle_step_bits, 2-byte aligned — ARCLE_ERR_ARG otherwise; bits
 * at cell indices >= H*W are ignored) with op int32 [..]; action_row_stride = 0: ONE set of K actions applied to every row ([K]
 * arrays), = n_actions: a set per row ([n_rows][K]).  The `bits` array arcle_components_rows writes when called with max_comp == K is
 * a valid per-row `sel` as it stands (zero-filled by the caller: entries of components that do not exist are not written; give their
 * slots an out-of-range op).  Int8 masks (ARCLE_INGRESS_MASK) and ARCLE_INGRESS_BBOX5 are not served here (ARCLE_ERR_ARG).  Outputs, all [n_rows][K], child c = m * K + k: reward int32, term uint8, status uint8 (the ARCLE_ST_* bits
 * child c raised), hash uint64 [..][2], optional dense int32 [..][2] (non-NULL implies ARCLE_STEP_DENSE: correct cells, total cells
 * of the child's grid against the answer of env src_env[m]), optional parent_hash uint64 [n_rows][2].  flags: ARCLE_STEP_RESET_ON_SUBMIT
 * | _DENSE.  For every (m, k) the outputs equal what arcle_transition_rows reports for (row m, action (m, k), src_env[m], same flags)
 * — reward, terminated, the tail's status byte, the dense pair — and hash equals arcle_hash_rows of the row that call would have
 * written.  No child row is written anywhere, and the handle's sticky status word, resident envs, counters, dense cache and installed
 * outputs are not touched.  Handles of more than ARCLE_MAX_CELLS cells per plane: ARCLE_ERR_CONFIG.  Allocates nothing: may be captured. */
int arcle_hash_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, uint64_t* hash, void* stream);
int arcle_expand_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t n_actions, int ingress,
                      const void* sel, const int32_t* op, int32_t action_row_stride, const int32_t* src_env, int32_t* reward,
                      uint8_t* term, uint8_t* status, uint64_t* hash, int32_t* dense, uint64_t* parent_hash, uint32_t flags,
                      void* stream);
/* arcle_expand_macros: K = n_actions MACROS per state row, a macro being a sequence of up to T = max_len steps; nothing but one set of
 * verdicts per macro is written.  sel is [..][K][T][w] (w = 4 int32 for ARCLE_INGRESS_BBOX, 2 int32 for ARCLE_INGRESS_POINT,
 * arcle_mask_bits_stride() bytes for ARCLE_INGRESS_BITS) and op int32 [..][K][T]; len int32 [..][K] = the steps macro k runs (steps
 * len .. T-1 of its slot are not read), NULL: every macro runs T; action_row_stride = 0: ONE set of K macros for every row, = n_actions:
 * a set per row, which sel, op and len all follow.  For every (m, k) the outputs equal what len[m, k] successive IN-PLACE
 * arcle_transition_rows calls report for (row m, steps 0 .. len-1 of macro (m, k), src_env[m], same flags): reward = the sum of the
 * steps' rewards, term = the last step's, status = the OR of the steps' status bits (a step that raises ARCLE_ST_BAD_OP or
 * _ROTATE_DOMAIN did not happen; the steps after it still run), dense = the pair the last step reports ((0, 0) if that step did not
 * happen), hash = arcle_hash_rows of the final row.  With max_len = 1 and len NULL the call is arcle_expand_rows, output for output.
 * A len outside [1, T] gives that child ARCLE_ST_BAD_OP and runs no step: its hash is the parent's, reward, term and dense are 0 —
 * as for a row whose src_env names no env (ARCLE_ST_BAD_TASK).  Refusals as arcle_expand_rows: int8 masks and ARCLE_INGRESS_BBOX5,
 * bit rows that are not 2-byte aligned, flags other than ARCLE_STEP_RESET_ON_SUBMIT | _DENSE, max_len < 1 or n_rows * n_actions *
 * max_len >= 2^28 (ARCLE_ERR_ARG); handles of more than ARCLE_MAX_CELLS cells per plane (ARCLE_ERR_CONFIG).  Nothing of the handle is
 * touched — sticky status word, resident envs, counters, dense cache, installed outputs.  Allocates nothing: may be captured. */
int arcle_expand_macros(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t n_actions, int32_t max_len, int ingress,
                        const void* sel, const int32_t* op, const int32_t* len, int32_t action_row_stride, const int32_t* src_env,
                        int32_t* reward, uint8_t* term, uint8_t* status, uint64_t* hash, int32_t* dense, uint64_t* parent_hash,
                        uint32_t flags, void* stream);
/* Connected components (color.py:8-30: 4-connected, same colour, inside grid_dim) of the grid of every state row, each as a ready-made
 * BBoxWrapper / PointWrapper action: what a search proposes its candidate actions from (arcle_expand_rows takes a set per row).
 * rows == NULL: the resident envs 0 .. n_rows-1 (n_rows <= n_envs); else rows as for arcle_hash_rows (any alignment, stride >= the
 * row length); only the grid segment and grid_dim of a row are read.
 *   count int32 [n_rows][2] = (written, left)
 *   comp  int32 [n_rows][max_comp][8] = x0, y0, x1, y1, sx, sy, colour, cells
 *   bits  optional uint8 [n_rows][max_comp][arcle_mask_bits_stride()]: the component's cells in the layout of arcle_step_bits /
 *         arcle_pack_mask_bits (bit f & 7 of byte f >> 3, f = row * W + col)
 * Components come in ascending row-major index of their first cell, sx * W + sy; that cell is the seed: a valid PointWrapper action
 * and a FloodFill seed.  (x0, y0, x1, y1) is the inclusive bounding box in BBoxWrapper's order (rows x, columns y).  skip_color: -1
 * skips nothing; otherwise cells of that colour belong to no component (0: ARC's background).  left = the cells inside grid_dim, not
 * of skip_color, that are in no written component: 0 <=> the list is complete.  Entries k >= written are not written at all.
 * No side effects: the handle's resident state, sticky status, counters, dense cache and installed outputs are untouched.  Refusals
 * as arcle_hash_rows (more than ARCLE_MAX_CELLS cells per plane: ARCLE_ERR_CONFIG); max_comp outside [1, ARCLE_MAX_CELLS], a stride
 * below the row length or rows == NULL with n_rows > n_envs: ARCLE_ERR_ARG.  One wavefront per row; allocates nothing: may be captured. */
int arcle_components_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, int32_t skip_color,
                          int32_t* count, int32_t* comp, uint8_t* bits, void* stream);
/* The objects of the grid of every state row under a chosen notion of "object": arcle_components_rows with a `mode` and an optional
 * set of colours per object.  Everything arcle_components_rows promises holds — the layout of count / comp / bits, rows == NULL, the
 * order (ascending row-major index of the first cell, which is the seed: x0 == sx), `left`, entries k >= written not written at all,
 * the refusals, no side effects, no allocation (may be captured), one wavefront per row, at most ARCLE_MAX_CELLS cells.
 *   mode   0: the components of arcle_components_rows, output for output.  ARCLE_OBJ_ANY_COLOR: every cell inside grid_dim whose
 *          colour is not skip_color may join — multi-colour objects (with skip_color == -1 a full rectangle is ONE object).
 *          ARCLE_OBJ_DIAG: 8-connected, (x, y) ~ (x', y') iff max(|x - x'|, |y - y'|) == 1.  Both may be set; any other bit:
 *          ARCLE_ERR_ARG.  comp[..][6] is the SEED's colour in every mode.
 *   colors optional uint32 [n_rows][max_comp]: bit v & 31 is set for every cell of the object, v the cell's byte taken as unsigned
 *          (for ARC's colours 0-9: the set of colours present; exactly one bit without ARCLE_OBJ_ANY_COLOR).  Entries k >= written
 *          are not written. */
#define ARCLE_OBJ_ANY_COLOR 1u
#define ARCLE_OBJ_DIAG 2u
int arcle_objects_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, int32_t skip_color,
                       uint32_t mode, int32_t* count, int32_t* comp, uint8_t* bits, uint32_t* colors, void* stream);
/* Where each object of a state row best fits the answer (ABI 12): for object k of row m — a bit row of arcle_components_rows /
 * arcle_objects_rows, taken as it stands — the translation whose Move macro (select the object, Move |dx| + |dy| times) leaves the
 * most correct cells, and that number, in closed form: no step is run.
 *   rows, stride  as for arcle_objects_rows (NULL: the resident envs 0 .. n_rows-1); only the grid and grid_dim are read
 *   count         int32 [n_rows][2] as arcle_objects_rows writes it: objects k >= count[m][0] are neither read nor written (the value is
 *                 clamped to [0, max_comp]); NULL: every row has max_comp objects
 *   bits          uint8 [n_rows][max_comp][arcle_mask_bits_stride()], 2-byte aligned
 *   src_env       int32 [n_rows]: the resident env whose answer plane and answer_dim judge row m, as arcle_expand_rows takes it (NULL:
 *                 env m, then n_rows <= n_envs)
 *   place         int32 [n_rows][max_comp][4] = dx, dy, correct(dx, dy), correct(0, 0)
 *   base          optional int32 [n_rows][2]: the dense pair (correct, total) of the row's own grid
 * With G the grid, (gh, gw) = min(grid_dim, (H, W)), A and (ah, aw) the answer of the env, B the cells of the bit row inside
 * [0, gh) x [0, gw) (bits outside it or at indices >= H * W are ignored) and (x0, y0, x1, y1) B's inclusive box, the candidates are
 *   T = {(dx, dy) : 0 <= x0 + dx, x1 + dx <= gh - 1, 0 <= y0 + dy, y1 + dy <= gw - 1, |dx| + |dy| <= max_dist}
 * (dx along rows, BBoxWrapper's x; the object stays wholly inside grid_dim; (0, 0) is always in T; B empty: T = {(0, 0)}).  The child
 * grid G'(dx, dy) at (x, y) is G[x - dx, y - dy] if that cell is in B and its byte, as int8, is > 0; else 0 if (x, y) is in B; else
 * G[x, y] — what the Moves leave (object.py:60-138, 218-243) — and correct(dx, dy) counts the cells of [0, min(gh, ah)) x
 * [0, min(gw, aw)) where G' equals A: the first number of the dense pair; the second does not change under a Move.  The best
 * translation maximises correct; ties go to the smaller |dx| + |dy|, then the smaller dx, then the smaller dy.  Any large max_dist
 * means no limit.  A row whose src_env names no env gets base = (0, 0) and place = (0, 0, 0, 0) for its objects.
 * No side effects, as arcle_objects_rows; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written:
 * max_comp outside [1, ARCLE_MAX_CELLS], n_rows <= 0, a stride below the row length, bits or place NULL, an odd bits address,
 * max_dist < 0, rows == NULL with n_rows > n_envs: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env kind without
 * an answer plane: ARCLE_ERR_CONFIG. */
int arcle_place_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                     const uint8_t* bits, const int32_t* src_env, int32_t max_dist, int32_t* place, int32_t* base, void* stream);
/* Where a COPY of each object of a state row best fits the answer (ABI 13): for object k of row m — a bit row as for arcle_place_rows —
 * the cell (px, py) at which CopyO + Paste (copy the object; paste the clip with its top-left corner at the selected cell) leaves the
 * most correct cells, and that number, in closed form: no step is run.
 *   rows, stride, count, bits, src_env, base, max_dist   as for arcle_place_rows (any large max_dist means no limit)
 *   blank         what the Paste of the caller's table does: 1 = it writes the clip's whole rectangle, zeros included (paste_blank, the
 *                 default tables' Paste: descriptor arg byte 1); 0 = only the clip's cells that are > 0
 *   stamp         int32 [n_rows][max_comp][4] = px, py, correct(px, py), the cells of B; entries k >= count are not written
 * With G the grid, (gh, gw) = min(grid_dim, (H, W)), A and (ah, aw) the answer of env src_env[m], (mh, mw) = min((gh, gw), (ah, aw)),
 * B the cells of the bit row inside [0, gh) x [0, gw) (bits outside it or at indices >= H * W are ignored), (x0, y0, x1, y1) B's
 * inclusive box and h x w its size, the clip is C[i, j] = G[x0 + i, y0 + j] if that cell is in B, else 0 (object.py:291-312), and the
 * candidates are
 *   T = {(px, py) : 0 <= px < gh, 0 <= py < gw, |px - x0| + |py - y0| <= max_dist}
 * — the top-left corner lies inside grid_dim; the stamp may hang over the bottom or the right edge and is then cut at the PLANE's
 * H x W, not at grid_dim (object.py:340-341); it never hangs over the top or the left.  The child G'(px, py) equals G except on
 * [px, min(px + h, H)) x [py, min(py + w, W)), where with blank = 1 G' = C[x - px, y - py], and with blank = 0 the same only where
 * C[x - px, y - py] > 0 as int8.  correct(px, py) counts the cells of [0, mh) x [0, mw) where G' equals A.  The best candidate
 * maximises correct; ties go to the smaller |dx| + |dy| with (dx, dy) = (px - x0, py - y0), then the smaller dx, then the smaller dy.
 * With blank = 1, (x0, y0) is a real edit: it zeroes the box's cells that are not in B.  B empty: (0, 0, base correct, 0).  A row
 * whose src_env names no env gets base = (0, 0) and stamp = (0, 0, 0, 0) for its objects.
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: those of arcle_place_rows,
 * and blank outside {0, 1}: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env kind without an answer plane:
 * ARCLE_ERR_CONFIG. */
int arcle_stamp_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                     const uint8_t* bits, const int32_t* src_env, int32_t max_dist, int32_t blank, int32_t* stamp, int32_t* base,
                     void* stream);
/* Where each object of a state row best fits the answer AFTER A TURN (ABI 14): for object k of row m — a bit row as for
 * arcle_place_rows — and each turn asked for, the translation at which select + turn + Moves (select the object with the turn's op, then
 * Move |dx| + |dy| times) leaves the most correct cells, and that number, in closed form: no step is run.
 *   rows, stride, count, bits, src_env, base, max_dist   as for arcle_place_rows (any large max_dist means no limit)
 *   turns         the set of turns asked for, ARCLE_TURN_* bits
 *   turn          int32 [n_rows][max_comp][5][4] = dx, dy, correct, valid; slot t is bit t of the masks below.  Slots of turns not in
 *                 `turns`, and of objects k >= count, are not written
 * G, (gh, gw), A, (ah, aw), (mh, mw), B and its inclusive box (x0, y0, x1, y1) of size h x w are as for arcle_place_rows.  O is the
 * h x w tile: O[i, j] = G[x0 + i, y0 + j] if that cell is in B, else 0.  For turn t, O_t is np.rot90(O, k) for the rotations by 90 k
 * degrees, np.fliplr(O) for FLIP_H and np.flipud(O) for FLIP_V; its size h' x w' is (w, h) for ROT90 / ROT270, else (h, w).  The corner
 * at which the turn leaves a freshly selected object is (nx, ny): (x0, y0) for ROT180, FLIP_H and FLIP_V; (floor((2 x0 + h - w) / 2),
 * floor((2 y0 + w - h) / 2)) for ROT90 / ROT270 (object.py:186-207 with rotation_parity = 0: both parity branches reduce to it).  The
 * candidates are
 *   T_t = {(dx, dy) : 0 <= nx + dx, nx + dx + h' <= gh, 0 <= ny + dy, ny + dy + w' <= gw, |dx| + |dy| <= max_dist}
 * — the turned tile lies wholly inside grid_dim, |dx| + |dy| Moves after the turn.  T_t may be empty (h > gw; or the tile overhangs at
 * (nx, ny) and max_dist is too small), and (0, 0) is in T_t only when the turn leaves the tile inside grid_dim.  The child G'(t, dx, dy)
 * is the background — G with B's cells zeroed — with the cells of O_t whose byte, as int8, is > 0 written at (nx + dx + i, ny + dy + j):
 * what select + turn + Moves leave (object.py:113-138, 167-279).  correct counts the cells of [0, mh) x [0, mw) where G' equals A; the
 * total does not change.  Per turn the best candidate maximises correct; ties go to the smaller |dx| + |dy|, then the smaller dx, then
 * the smaller dy (arcle_place_rows' rule); valid = 1.  T_t empty: the slot is (0, 0, 0, 0).  B empty: (0, 0, base correct, 1) for every
 * turn asked for.  A row whose src_env names no env gets base = (0, 0) and zeros.
 * The diagonal flips (D0 / D1) are out of scope: the reference leaves object_dim untransposed for them (object.py:270-273), so their
 * child is a truncated tile, not a turn of the object.
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: those of arcle_place_rows,
 * and turns == 0 or a bit above ARCLE_TURN_FLIP_V: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env kind without an
 * answer plane: ARCLE_ERR_CONFIG. */
#define ARCLE_TURN_ROT90 1u   /* gen_rotate(1) */
#define ARCLE_TURN_ROT180 2u  /* gen_rotate(2) */
#define ARCLE_TURN_ROT270 4u  /* gen_rotate(3) */
#define ARCLE_TURN_FLIP_H 8u  /* gen_flip("H") */
#define ARCLE_TURN_FLIP_V 16u /* gen_flip("V") */
int arcle_turn_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                    const uint8_t* bits, const int32_t* src_env, int32_t max_dist, uint32_t turns, int32_t* turn, int32_t* base,
                    void* stream);
/* The offset at which the GRID or the INPUT of a state row best fits the ANSWER'S CANVAS (ABI 15): for row m and each source asked for,
 * the offset (ox, oy) at which the three-step macro
 *   [Copy_src on R, resize_grid on the rectangle (0, 0)..(ah - 1, aw - 1), Paste on the single cell P]
 * leaves the most correct cells, and that number, in closed form: no step is run.  The only sibling whose child has another grid_dim
 * than its row: the macro leaves grid_dim = (ah, aw), so a task whose answer has another size than the grid can be solved.
 *   rows, stride, src_env, base, stream   as for arcle_place_rows (rows NULL: the resident envs, n_rows <= n_envs).  There are no
 *                 objects: no count, no bits.  Of a row only grid, grid_dim, input and input_dim are read
 *   max_dist      offsets with |ox| + |oy| <= max_dist (any large max_dist means no limit)
 *   sources       the set of sources asked for, ARCLE_ALIGN_* bits
 *   blank         the paste_blank of the caller's Paste: 1 writes the clip's whole rectangle, 0 its positive cells only
 *   align         int32 [n_rows][2][8] = ox, oy, correct, total, sh, sw, ah, aw; slot 0 is the grid, slot 1 the input.  Slots of sources
 *                 not in `sources` are not written
 * S is the source plane — the row's grid (ARCLE_ALIGN_GRID, copied by Copy_O, object.py:291-312) or the row's input (ARCLE_ALIGN_INPUT,
 * copied by Copy_I, critical.py:39-46) — and (sh, sw) = min(its dim, (H, W)), clamped at 0; A is the answer of env src_env[m] and
 * (ah, aw) = min(its answer_dim, (H, W)).  The candidates are
 *   T = {(ox, oy) : -ah < ox < sh, -aw < oy < sw, |ox| + |oy| <= max_dist}
 * — the copied rectangle R = [max(ox, 0), min(sh, ah + ox)) x [max(oy, 0), min(sw, aw + oy)) is never empty; (0, 0) is in T whenever
 * all four dims are >= 1, and T is empty only when a dim is 0: the slot is then (0, 0, 0, 0, sh, sw, ah, aw).  resize_grid leaves an
 * all-zero ah x aw grid, and Paste on P = (max(-ox, 0), max(-oy, 0)) writes the clip with its corner there, cut at the plane
 * (object.py:340-348).  The child G'(ox, oy) is, for (i, j) in the canvas [0, ah) x [0, aw),
 *   G'[i, j] = S[i + ox, j + oy]  if (i + ox, j + oy) lies inside (sh, sw) (blank = 0: and that byte, as int8, is > 0), else 0
 * and 0 elsewhere on the plane: source bytes outside the source's dims are never read as anything but 0; with blank = 1 negative source
 * bytes are carried over, with blank = 0 they become 0.  ox, oy >= 0 with full cover is "the answer is a window of the source";
 * ox, oy <= 0 is "the source embedded in a larger canvas"; everything in between is a partial overlap.  correct(ox, oy) counts the
 * cells of the canvas where G' equals A; total = ah * aw is the child's dense total (its dims equal the answer's), so the child is a
 * goal exactly when correct == total.  The best offset maximises correct; ties go to the smaller |ox| + |oy|, then the smaller ox,
 * then the smaller oy (arcle_place_rows' rule).  base is the dense pair of the row's own grid, as the siblings write it.  A row whose
 * src_env names no env gets base = (0, 0) and all-zero slots.
 * A one-step crop_grid form, turned sources and the objects of the input are out of scope (zoomed, shrunk and tiled sources:
 * arcle_scale_rows).
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: n_rows <= 0, a stride below
 * the row length, align NULL, max_dist < 0, sources == 0 or a bit above ARCLE_ALIGN_INPUT, blank outside {0, 1}, rows == NULL with
 * n_rows > n_envs (with or without src_env: row m's grid is env m's): ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an
 * env kind without an answer plane: ARCLE_ERR_CONFIG. */
#define ARCLE_ALIGN_GRID 1u  /* source = the row's grid (Copy_O) */
#define ARCLE_ALIGN_INPUT 2u /* source = the row's input (Copy_I) */
int arcle_align_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, const int32_t* src_env, int32_t max_dist,
                     uint32_t sources, int32_t blank, int32_t* align, int32_t* base, void* stream);
/* The LINES each object of a state row casts toward the answer (ABI 16): for object k of row m — a bit row as for arcle_place_rows — and
 * each of n_sets sets of directions, the cells its rays cover, the colour c for which ONE `Color c` step on exactly those cells
 * (color.py:70-77) leaves the most correct cells, and that number, in closed form: no step is run.  The only sibling that draws: the
 * child holds cells that no object of the row holds ("extend every pixel to the border", "shoot a line until it hits a wall", "a cross
 * or a star through each seed").
 *   rows, stride, max_comp, count, bits, src_env, base, stream   as for arcle_place_rows
 *   sets          uint8 [n_sets], 1 <= n_sets <= 16, the same for all rows: DEVICE memory, read by the kernel when the launch runs (like
 *                 the op table: a captured launch sees the bytes it holds at replay).  Entry s is a mask of ARCLE_RAY_* directions; a
 *                 zero entry is allowed and is the empty candidate
 *   free_color    through = 0: the int8 byte of the cells a ray may enter, -128 .. 127 (callers pass 0: the background)
 *   through       0: a ray stops in front of the first cell whose byte is not free_color; 1: it runs over every cell to the edge
 *   ray           int32 [n_rows][max_comp][n_sets][4] = color, correct, cells, right; slots of objects k >= count are not written
 *   best          int32 [n_rows][max_comp][4] = set, color, correct, cells; likewise
 *   best_bits     optional uint8 [n_rows][max_comp][arcle_mask_bits_stride()], 2-byte aligned: the best candidate's cells in the bit-row
 *                 format of arcle_expand_rows / arcle_transition_rows (ARCLE_INGRESS_BITS) — the selection of the step, made on the
 *                 device; all arcle_mask_bits_stride() bytes of a written slot are written
 * BOARDS.  G is the row's grid, (gh, gw) = min(grid_dim, (H, W)); A and (ah, aw) = min(answer_dim, (H, W)) are the answer of env
 * src_env[m]; (mh, mw) = min((gh, gw), (ah, aw)) is the common rectangle; B is the cells of the bit row inside [0, gh) x [0, gw) (bits
 * outside it or at indices >= H * W are ignored).  x runs along rows (down), y along columns, as everywhere in this ABI.
 * DIRECTIONS.  Bit 0..7 of a mask: N (-1, 0), S (+1, 0), W (0, -1), E (0, +1), NW (-1, -1), NE (-1, +1), SW (+1, -1), SE (+1, +1) as
 * (dx, dy).  shift_d(X) = {(x + dx, y + dy) : (x, y) in X}.
 * FREE CELLS.  F = the cells of [0, gh) x [0, gw) that are not in B and, with through = 0, whose grid byte equals free_color as int8;
 * with through = 1, all of them.
 * RAY.  R_d is the least board with R_d = shift_d(B | R_d) & F: walk from every cell of B in direction d and take cells while they are
 * in F.  A ray starts only next to B's own cells (it does not jump a gap), stops in front of the first cell that is not free or at the
 * edge of grid_dim, and never wraps from one row or column into the next.  Cells of B never belong to a ray; a ray may cross a hole
 * that B encloses only where the hole's cells are free, and goes on behind a further cell of B only as that cell's own ray.
 * CANDIDATES.  Candidate s of an object is R_s = the union of R_d over the directions d in sets[s]; its step is ONE `Color c` on the
 * selection R_s, whose child is G with R_s's cells set to c: grid_dim and the dense total do not change.  With K = the cells of the
 * common rectangle at which G equals A,
 *   cells   = |R_s|
 *   right   = max over c in 0..9 of |{(x, y) in R_s, inside the common rectangle, A[x, y] == c}|,  color = the smallest c reaching it
 *   correct = base correct - |R_s & K| + right      — the first number of the child's dense pair
 * and an empty R_s (a zero set, an empty B, no free neighbour) gives the slot (0, base correct, 0, 0).
 * BEST.  Among the candidates with cells > 0 the one with the most correct; ties go to fewer cells, then to the lower set index:
 * (set, color, correct, cells) and R_set in best_bits.  If every candidate is empty: (-1, 0, base correct, 0) and an all-zero bit row.
 * base is the dense pair of the row's own grid, as the siblings write it.  A row whose src_env names no env gets base = (0, 0) and
 * zeros in all slots of its objects (ray, best and best_bits).
 * Out of scope: handles of more than ARCLE_MAX_CELLS cells; a limit on a ray's length; rays of more than one colour or of a colour
 * no single Color step gives (a ray that takes its object's colour is `Color` of that colour: it is scored, but only the best c is
 * reported); rays started from the cells of the INPUT instead of the grid's objects.
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: those of arcle_place_rows
 * (without max_dist), sets, ray or best NULL, n_sets outside [1, 16], an odd best_bits address, through outside {0, 1}, free_color
 * outside [-128, 127]: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env kind without an answer plane:
 * ARCLE_ERR_CONFIG. */
#define ARCLE_RAY_N 1u
#define ARCLE_RAY_S 2u
#define ARCLE_RAY_W 4u
#define ARCLE_RAY_E 8u
#define ARCLE_RAY_NW 16u
#define ARCLE_RAY_NE 32u
#define ARCLE_RAY_SW 64u
#define ARCLE_RAY_SE 128u
int arcle_ray_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                   const uint8_t* bits, const int32_t* src_env, const uint8_t* sets, int32_t n_sets, int32_t free_color,
                   int32_t through, int32_t* ray, int32_t* best, uint8_t* best_bits, int32_t* base, void* stream);
/* Each object's box filled from its MIRROR IMAGE (ABI 17): for object k of row m — a bit row as for arcle_place_rows — and each symmetry
 * asked for, the source rectangle whose flipped copy, written over the object's box, leaves the most correct cells: the repair of a
 * symmetric pattern with a hole punched out.  It is what the step sequence CopyO on R, Paste at the box's corner, Flip of the box leaves.
 * rows, stride, count, bits, src_env, base and stream as for arcle_turn_rows.
 *   mirrors       the set of symmetries asked for, ARCLE_MIRROR_* bits
 *   blank         what the table's Paste does: 1 = the clip's whole rectangle is written (paste_blank: both default tables), 0 = its
 *                 positive cells only
 *   mirror        int32 [n_rows][max_comp][3][4] = dx, dy, correct, valid; slot s is bit s of `mirrors`.  Slots of symmetries not in
 *                 `mirrors`, and of objects k >= count, are not written
 * G, (gh, gw), A, (ah, aw), (mh, mw) and B as for arcle_place_rows; (x0, y0, x1, y1) B's inclusive box of h x w cells.  A candidate of
 * slot s is a source rectangle R of h x w cells with its corner at (x0 + dx, y0 + dy), wholly inside grid_dim, |dx| + |dy| <= max_dist;
 * dx = 0 in slot H, dy = 0 in slot V, both free in slot POINT.  R may overlap the box, and dx = dy = 0 — the box flipped where it stands
 * — is always a candidate.  Let T be the h x w tile that Copy + Paste leave in the box: with blank = 1, T = G[R]; with blank = 0, T =
 * G[R] where G[R] > 0 and the box's own old cell elsewhere.  The child G'(s, dx, dy) is G with the box replaced by pos(flip_s(T)), flip_s
 * = np.fliplr (H), np.flipud (V) or both (POINT), pos(v) = v if v > 0 else 0: the Flip lifts the whole rectangle as an object and writes
 * back its positive cells only (object.py:60-138, 265-276, 291-348).  Nothing outside the box changes.  correct counts the cells of [0,
 * mh) x [0, mw) where G' equals A; the total does not change.  Per slot the best candidate maximises correct; ties go to the smaller |dx|
 * + |dy|, then the smaller dx, then the smaller dy: (dx, dy, correct, 1).  A slot without a candidate: (0, 0, 0, 0).  An empty B:
 * (0, 0, base correct, 1) in every slot asked for.  A row whose src_env names no env gets base = (0, 0) and zeros.
 * Out of scope: the diagonal symmetries (Flip D0 / D1 leave object_dim unswapped for non-square boxes, and the default tables carry
 * neither op), the input plane as a source (CopyI), handles of more than ARCLE_MAX_CELLS cells.
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: those of arcle_place_rows,
 * mirrors == 0 or a bit above ARCLE_MIRROR_POINT, blank outside {0, 1}: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an
 * env kind without an answer plane: ARCLE_ERR_CONFIG. */
#define ARCLE_MIRROR_H 1u     /* columns mirrored: what gen_flip("H") (np.fliplr) does to the pasted box */
#define ARCLE_MIRROR_V 2u     /* rows mirrored: gen_flip("V") (np.flipud) */
#define ARCLE_MIRROR_POINT 4u /* both: the point reflection (= a half turn) */
int arcle_mirror_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                      const uint8_t* bits, const int32_t* src_env, int32_t max_dist, uint32_t mirrors, int32_t blank, int32_t* mirror,
                      int32_t* base, void* stream);
/* The cells AROUND and INSIDE each object of a state row (ABI 18): for object k of row m — a bit row as for arcle_place_rows — and each
 * of n_kinds kinds of region, the region's cells, the colour c for which ONE `Color c` step on exactly those cells (color.py:70-77)
 * leaves the most correct cells, and that number, in closed form: no step is run.  A sibling of arcle_ray_rows, which draws straight
 * lines: "outline every object", "fill the inside of every closed shape", "fill the rest of the bounding box", "a frame round the box"
 * are one step each.
 *   rows, stride, max_comp, count, bits, src_env, base, stream   as for arcle_place_rows
 *   kinds         uint8 [n_kinds], 1 <= n_kinds <= 16, the same for all rows: DEVICE memory, read by the kernel when the launch runs
 *                 (like the `sets` of arcle_ray_rows: a captured launch sees the bytes it holds at replay).  Entry s is an
 *                 ARCLE_REGION_* code.  ARCLE_REGION_NONE is allowed and is the empty candidate.  Because the array lives on the
 *                 device, this entry point cannot see its codes: a code above 7 is NOT refused, the kernel takes it as
 *                 ARCLE_REGION_NONE
 *   free_color    through = 0: the int8 byte a cell OUTSIDE the object must hold to be painted, -128 .. 127 (callers pass 0: the
 *                 background)
 *   through       0: the free filter applies; 1: every cell of the region is painted
 *   region        int32 [n_rows][max_comp][n_kinds][4] = color, correct, cells, right; slots of objects k >= count are not written
 *   best          int32 [n_rows][max_comp][4] = index (into kinds), color, correct, cells; likewise
 *   best_bits     optional uint8 [n_rows][max_comp][arcle_mask_bits_stride()], 2-byte aligned: the best candidate's cells in the bit-row
 *                 format of arcle_expand_rows / arcle_transition_rows (ARCLE_INGRESS_BITS); all arcle_mask_bits_stride() bytes of a
 *                 written slot are written
 * BOARDS.  G, (gh, gw), A, (ah, aw), (mh, mw) and B as for arcle_ray_rows: B is the cells of the bit row inside IN = [0, gh) x [0, gw)
 * (bits outside it or at indices >= H * W are ignored).  FREE = the cells of IN whose grid byte equals free_color as int8; with through
 * = 1, FREE = IN.  box = the bounding rectangle [x0, x1] x [y0, y1] of B, computed from B (not passed in).
 * REGIONS.
 *   ARCLE_REGION_NONE       empty
 *   ARCLE_REGION_HALO4      the cells of IN & ~B with a 4-neighbour in B
 *   ARCLE_REGION_HALO8      the cells of IN & ~B with an 8-neighbour in B
 *   ARCLE_REGION_BOX_REST   box & ~B
 *   ARCLE_REGION_BOX_FRAME  [x0 - 1, x1 + 1] x [y0 - 1, y1 + 1] minus box, clipped to IN
 *   ARCLE_REGION_INSIDE     the cells of IN & ~B from which no path of 4-connected steps through IN & ~B leads to a cell on the edge
 *                           of grid_dim (row 0 or gh - 1, column 0 or gw - 1).  An edge cell is never inside: the grid's edge does not
 *                           close a shape.  A ring whose cells touch only diagonally does enclose: the path is 4-connected
 *   ARCLE_REGION_BOX        box, B's cells included
 *   ARCLE_REGION_SELF       B
 * An empty B has no box: all its regions are empty.  Nothing lies outside IN and nothing wraps from one row or column into the next.
 * CANDIDATES.  Candidate s of an object is R_s = region(kinds[s]) & (B | FREE): the free filter applies to the cells outside the object
 * only.  Its step is ONE `Color c` on the selection R_s, whose child is G with R_s's cells set to c: grid_dim and the dense total do not
 * change.  With K = the cells of the common rectangle at which G equals A,
 *   cells   = |R_s|   (up to H * W: BOX or SELF of an object that is the whole grid)
 *   right   = max over c in 0..9 of |{(x, y) in R_s, inside the common rectangle, A[x, y] == c}|,  color = the smallest c reaching it
 *   correct = base correct - |R_s & K| + right      — the first number of the child's dense pair
 * and an empty R_s gives the slot (0, base correct, 0, 0).
 * BEST.  Among the candidates with cells > 0 the one with the most correct; ties go to fewer cells, then to the lower index:
 * (index, color, correct, cells) and R_index in best_bits.  If every candidate is empty: (-1, 0, base correct, 0) and an all-zero bit
 * row.  base is the dense pair of the row's own grid, as the siblings write it.  A row whose src_env names no env gets base = (0, 0) and
 * zeros in all slots of its objects (region, best and best_bits).
 * Out of scope: handles of more than ARCLE_MAX_CELLS cells; halos wider than one cell; the inside under 8-connected paths; regions of
 * more than one colour (only the best c of each is reported).
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: those of arcle_ray_rows with
 * kinds / n_kinds / region in the place of sets / n_sets / ray (kinds, region or best NULL, n_kinds outside [1, 16], an odd best_bits
 * address, through outside {0, 1}, free_color outside [-128, 127]: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env
 * kind without an answer plane: ARCLE_ERR_CONFIG). */
#define ARCLE_REGION_NONE 0u
#define ARCLE_REGION_HALO4 1u
#define ARCLE_REGION_HALO8 2u
#define ARCLE_REGION_BOX_REST 3u
#define ARCLE_REGION_BOX_FRAME 4u
#define ARCLE_REGION_INSIDE 5u
#define ARCLE_REGION_BOX 6u
#define ARCLE_REGION_SELF 7u
int arcle_region_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, int32_t max_comp, const int32_t* count,
                      const uint8_t* bits, const int32_t* src_env, const uint8_t* kinds, int32_t n_kinds, int32_t free_color,
                      int32_t through, int32_t* region, int32_t* best, uint8_t* best_bits, int32_t* base, void* stream);
/* The grid or the input of a state row zoomed, shrunk or tiled onto the answer's canvas: an EXTENSION of ABI 18, declared in a header of
 * its own.  ARCLE_ABI_VERSION and the entry points declared in this file stay as they are; a library that carries the extension defines
 * ARCLE_HAS_SCALE_ROWS there and exports its one entry point beside these. */
#include "arcle_scale_rows.h"
/* One state plane as a dense [n_envs][H*W] int8 array (device or pinned host memory), a strided copy on the stream: the
 * get_state()/set_state() of single keys of the reference's state dict. */
int arcle_get_plane(arcle_env* env, int plane, int8_t* dst, void* stream);
int arcle_set_plane(arcle_env* env, int plane, const int8_t* src, void* stream);

/* Packed minimal observation for a central learner (what the multi-GPU gather moves): one row per env,
 *   grid (H*W bytes) | grid_dim (2) | reward int32 little-endian (4) | terminated (1) | zero padding
 * of arcle_packed_obs_size() bytes (H*W + 7 rounded up to 16; 912 for 30x30).  reward / term are the arrays the last step
 * wrote; out is a device buffer uint8 [n_envs][arcle_packed_obs_size()], 16-byte aligned. */
int arcle_packed_obs_size(const arcle_env* env);
int arcle_pack_obs(arcle_env* env, const int32_t* reward, const uint8_t* term, uint8_t* out, void* stream);
/* destination of ARCLE_STEP_PACK_OBS: uint8 [n_envs][arcle_packed_obs_size()], 16-byte aligned (NULL uninstalls it) */
int arcle_set_packed_output(arcle_env* env, uint8_t* out);

/* Reads and (optionally) clears the sticky device status word (ARCLE_ST_*): one atomic exchange on the device, so a
 * bit raised by a kernel on another stream is never lost between the read and the clear.  Synchronises the stream.
 * Ordering of the setters (arcle_set_op_table, _task_table, _sampler, _truncation, _dense_output, _flat_output, _packed_output):
 * every launch takes its parameters — table pointers included — BY VALUE at the moment it is enqueued (or captured into a
 * hipGraph).  A setter therefore changes what LATER launches see and never what is already in flight or captured; the library's
 * own op-table copy is versioned (a new device buffer per arcle_set_op_table, the old ones are freed in arcle_destroy), and
 * caller-owned arrays (task table, sampler arrays, output buffers) must simply stay alive until the launches / graphs that were
 * given them have finished.  No setter synchronises. */
int arcle_get_status(arcle_env* env, uint32_t* status, int clear, void* stream);

/* Algorithmic HBM bytes (SURVEY.md §8d accounting) moved by all step launches (and the observation rows written by
 * arcle_flatten_obs / ARCLE_STEP_FLAT_OBS: planes + record read once, row written once) since the
 * last call with clear != 0; accumulated on device by the step kernel only when the handle
 * was created with accounting enabled via arcle_enable_accounting(env, 1). */
int arcle_enable_accounting(arcle_env* env, int on);
int arcle_get_accounting(arcle_env* env, uint64_t* bytes, uint64_t* steps, int clear, void* stream);
/* ... and next to the algorithmic figure `issued`: the bytes of every global-memory access the step kernel actually issued for
 * those steps (whole 16-byte lanes of every plane access incl. row padding, record / counters / action / outputs, observation rows,
 * task-table reads) — elided writes are not in it, re-reads are. */
int arcle_get_accounting_ex(arcle_env* env, uint64_t* bytes, uint64_t* issued, uint64_t* steps, int clear, void* stream);

const char* arcle_last_error(const arcle_env* env);
int arcle_abi_version(void);

/* (Diagnostic builds compiled with -DARCLE_TRACE_WAVES additionally export a per-wave timestamp dump used by tools/wavetrace.py; it does
 * not exist in the shipped library and is therefore not declared here.) */

#ifdef __cplusplus
}
#endif
#endif /* ARCLE_HIP_H */
