/* arcle_scale_rows.h — the one entry point of the "scale" extension of the arcle_hip C ABI.  Included by arcle_hip.h (inside its
 * extern "C" block, after arcle_env, the error codes, ARCLE_MAX_CELLS and the ARCLE_ALIGN_* bits it uses): include that file, not this
 * one.  The extension adds an entry point and changes none: ARCLE_ABI_VERSION stays 18, and a caller that needs the entry point asks
 * for ARCLE_HAS_SCALE_ROWS at compile time or looks the symbol up at run time. */
#ifndef ARCLE_SCALE_ROWS_H
#define ARCLE_SCALE_ROWS_H
#define ARCLE_HAS_SCALE_ROWS 1

/* The GRID or the INPUT of a state row ZOOMED, SHRUNK or TILED onto the ANSWER'S CANVAS (an extension of ABI 18): for row m and each source asked for,
 * the best of 132 separable cell maps, its correct cells, the colours of its child and that child's cells colour by colour, in closed
 * form: no step is run.  Like arcle_align_rows the child has grid_dim = (ah, aw), so tasks whose answer has another size than the grid
 * — "every cell becomes a k x k block", "every k x k block becomes one cell", "the input repeated n x m times, plain or mirrored" — can
 * be solved; arcle_align_rows never repeats or resamples a cell.
 *   rows, stride, src_env, base, stream, sources   as for arcle_align_rows (ARCLE_ALIGN_GRID: slot 0, the row's grid; ARCLE_ALIGN_INPUT:
 *                 slot 1, the row's input).  Of a row only grid, grid_dim, input and input_dim are read
 *   modes         the set of candidate families asked for, ARCLE_SCALE_* bits
 *   scale         int32 [n_rows][2][8] = cand, correct, total, colours, sh, sw, ah, aw.  Bit c (1..9) of colours is set iff colour c occurs
 *                 in the best child.  Slots of sources not in `sources` are not written (nor are their table and bits rows)
 *   table         optional int32 [n_rows][2][ARCLE_SCALE_CANDS]: correct of every candidate, -1 for candidates whose mode is not in `modes`
 *   bits          optional uint8 [n_rows][2][9][arcle_mask_bits_stride()], 2-byte aligned: row c - 1 holds the best child's cells of
 *                 colour c in the layout of arcle_step_bits; all nine rows are written
 * DIMS AND SOURCE VALUE.  (H, W) is the plane's size, S the source plane, (sh, sw) its dim clamped to [0, H] x [0, W]; A is the answer of
 * env src_env[m] and (ah, aw) = min(its answer_dim, (H, W)).  The source value is
 *   v(x, y) = S[x, y]  if 0 <= x < sh, 0 <= y < sw and 1 <= S[x, y] <= 9, else 0
 * — bytes outside the source's dims, negative bytes and bytes above 9 are read as 0: the macro below paints with Color steps, which can
 * write nothing else.
 * CANDIDATES.  Every candidate is a separable cell map: its child on the canvas [0, ah) x [0, aw) is G'[i, j] = v(f(i), g(j)), and 0
 * elsewhere on the plane; an index outside [0, sh) or [0, sw) reads 0 through v.
 *   (kx - 1) * 8 + (ky - 1), kx, ky in 1..8        ZOOM    f(i) = i div kx, g(j) = j div ky
 *   64 + (kx - 1) * 8 + (ky - 1)                   SHRINK  f(i) = i * kx, g(j) = j * ky (the top-left cell of each block)
 *   128 + t, t in 0..3                             TILE    period (sh, sw); bit 0 of t mirrors every second tile column: g(j) =
 *                                                          sw - 1 - (j mod sw) when (j div sw) is odd, else j mod sw; bit 1 of t does
 *                                                          the same for the tile rows
 * SCORING.  correct(c) counts the canvas cells where G' equals A as bytes (an answer byte outside 0..9 never matches); total = ah * aw
 * is the child's dense total, since its dims are the answer's: the child is a goal exactly when correct == total.  The best candidate
 * maximises correct over the modes asked for; ties go to the lowest index (ZOOM(1, 1) beats SHRINK(1, 1) and TILE 0; a constant source
 * reports index 0).
 * NO CANDIDATE: a slot one of whose sh, sw, ah, aw is 0 has cand -1, correct 0, total 0, colours 0, then the four dims; its table row is
 * all -1, its bits rows all zero.  A row whose src_env names no env gets such slots with all four dims 0, and base = (0, 0).
 * THE MACRO that realises a candidate is [resize_grid on the rectangle (0, 0)..(ah - 1, aw - 1), then Color c on the child's cells of
 * colour c, for each colour present, ascending]: 1 + popcount(colours) steps, at most 10.  resize_grid leaves an all-zero ah x aw grid
 * (critical.py:31-46), so colour 0 needs no step, and a Color step on exactly those cells writes exactly them (color.py:70-77).
 * Out of scope: majority down-sampling, rotated tiles, the Kronecker product of the source with itself, mixed zoom and shrink across
 * the two axes; handles of more than ARCLE_MAX_CELLS cells.
 * No side effects; allocates nothing: may be captured.  One wavefront per row.  Refusals, nothing written: n_rows <= 0, a stride below
 * the row length, scale NULL, an odd bits address, sources == 0 or a bit above ARCLE_ALIGN_INPUT, modes == 0 or a bit above
 * ARCLE_SCALE_TILE, rows == NULL with n_rows > n_envs: ARCLE_ERR_ARG; more than ARCLE_MAX_CELLS cells per plane, or an env kind
 * without an answer plane: ARCLE_ERR_CONFIG. */
#define ARCLE_SCALE_ZOOM 1u   /* every source cell becomes a kx x ky block */
#define ARCLE_SCALE_SHRINK 2u /* the top-left cell of every kx x ky block */
#define ARCLE_SCALE_TILE 4u   /* the source repeated, plain or with mirrored tile columns / rows */
#define ARCLE_SCALE_CANDS 132
int arcle_scale_rows(arcle_env* env, int32_t n_rows, const int8_t* rows, int32_t stride, const int32_t* src_env, uint32_t sources,
                     uint32_t modes, int32_t* scale, int32_t* table, uint8_t* bits, int32_t* base, void* stream);

#endif /* ARCLE_SCALE_ROWS_H */
