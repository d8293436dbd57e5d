/* bm355.h — C-ABI of libbm355.so, the MI355X (gfx950) RBM/DBM engine.
 *
 * The reference (yell/boltzmann-machines) has no FFI: its only seam is
 * Python class API <-> `session.run`.  Every entry point
 * below replaces one `session.run` / `.eval` fetch site of the reference,
 * cited as  reference-file:line  next to the declaration.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message
 *     is available from bm_last_error() (thread-local).
 *   - `*_dev` pointers are DEVICE pointers (hipMalloc / bm_dev_alloc /
 *     torch .data_ptr()); everything else is host memory owned by the caller.
 *   - a handle owns all model state (W, biases, momentum buffers, running
 *     means, chain workspaces) in HBM and one HIP stream; calls on one handle
 *     are asynchronous on that stream and must not be issued concurrently
 *     from several host threads.  bm_*_sync() blocks until the stream drains.
 *   - a failed bm_*_create (bm_rbm, bm_rbm64, bm_dbm, bm_dbm64) frees everything
 *     it had allocated and leaves *out untouched; bm_*_destroy(NULL) is a no-op.
 *   - all arithmetic is fp32 (reference default dtype, base/mixin.py:15).
 *   - matrices are row-major; W is [n_below, n_above] like the reference
 *     (base_rbm.py:277-293).
 */
#ifndef BM355_H
#define BM355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ misc */
const char *bm_last_error(void);
/* "bm355 <version> gfx950" */
const char *bm_version(void);
/* number of visible HIP devices (0 when no GPU / no driver) */
int bm_device_count(void);
int bm_set_device(int device);

/* raw device-memory helpers so that a host without torch can drive the ABI */
int bm_dev_alloc(size_t bytes, void **out_dev);
int bm_dev_free(void *dev);
int bm_h2d(void *dst_dev, const void *src_host, size_t bytes);
int bm_d2h(void *dst_host, const void *src_dev, size_t bytes);
int bm_dev_memset(void *dst_dev, int value, size_t bytes);

/* XCD-aware block -> tile map of the tile kernels (csrc/bm_gemm.h tile_of_block), evaluated on the host: for tests
 * and tools.  out_ti / out_tj: tile of every block of a tiles_i x tiles_j launch; out_map5 = {xi, xj, gj, tiles_i, tiles_j} */
int bm_debug_tile_map(int32_t tiles_i, int32_t tiles_j, double bytes_i, double bytes_j, int32_t *out_ti,
                      int32_t *out_tj, int32_t *out_map5);

/* ------------------------------------------------------------------- RBM */
typedef struct bm_rbm bm_rbm;

/* BM_UNIT_NRELU: noisy rectified-linear HIDDEN units (Nair & Hinton 2010; no counterpart in the reference).  With
 * t = v W + hb in float32: mean max(0, t), state max(0, t + n sqrt(sigmoid(t))), n a standard normal draw by position - the
 * sigmoid of csrc/bm_numerics.h, a correctly rounded square root, one rounded multiply and one rounded add (no fused
 * multiply-add).  bm_rbm_config.h_unit only, with Bernoulli or Gaussian visible units.  Such a handle trains (train_step,
 * _metrics, _metrics_async, _epoch), transforms, runs bm_rbm_gibbs / bm_rbm_metrics / bm_rbm_sample_h and is staged like any
 * other; out4[1] (pll) and out4[3] (free energy) of the metric calls are NaN - the unit has no closed-form free energy.  Refused,
 * with a message that names NReLU: dbm_first / dbm_last, sparsity_cost != 0 and dropout (at create); bm_rbm_free_energy(_rows),
 * bm_rbm_ais, bm_rbm_pt_*, bm_rbm_train_step_pt / _epoch_pt, bm_rbm_set_fast_weights, bm_rbm_set_centering, bm_rbm_set_classes
 * and every bm_rbm_class_* entry, bm_rbm_gibbs_clamped, bm_rbm_grad_step / _apply_step and the gradient exchange entries,
 * bm_rbm_backprop_down / _delta_update / the stack entries, bm_rbm64_create.  bm_rbm_set_fast_binary is accepted and runs fp32. */
enum { BM_UNIT_BERNOULLI = 0, BM_UNIT_GAUSSIAN = 1, BM_UNIT_MULTINOMIAL = 2, BM_UNIT_NRELU = 3 };

/* ctor kwargs of BaseRBM.__init__ that influence the device graph
 * (rbm/base_rbm.py:95-105, :244-327). */
typedef struct bm_rbm_config {
    int32_t n_visible;
    int32_t n_hidden;
    int32_t v_unit;            /* BM_UNIT_*: BernoulliRBM / GaussianRBM (rbm/rbm.py:10-15,88-99) */
    int32_t sample_v_states;   /* base_rbm.py:100 */
    int32_t sample_h_states;   /* base_rbm.py:100 */
    int32_t dbm_first;         /* propup multiplier 1+dbm_first (base_rbm.py:256-260) */
    int32_t dbm_last;          /* propdown multiplier 1+dbm_last (base_rbm.py:261-262) */
    int32_t max_batch;         /* largest minibatch the workspaces must hold */
    float   l2;                /* base_rbm.py:249 */
    float   sparsity_target;   /* base_rbm.py:253-255 */
    float   sparsity_cost;
    float   sparsity_damping;
    float   dropout;           /* keep-prob of tf.nn.dropout; <0 => no dropout (base_rbm.py:417-418) */
    int32_t h_unit;            /* BM_UNIT_BERNOULLI, or BM_UNIT_MULTINOMIAL = MultinomialRBM (rbm/rbm.py:25-65,
                                  layers.py:54-70): means = n_samples*softmax, states = multinomial counts */
    int32_t n_samples;         /* MultinomialLayer.n_samples (rbm.py:46); ignored for Bernoulli hidden units */
} bm_rbm_config;

/* on failure nothing stays allocated and *out is not written (the same for bm_rbm64 / bm_dbm / bm_dbm64_create) */
int bm_rbm_create(const bm_rbm_config *cfg, bm_rbm **out);
int bm_rbm_destroy(bm_rbm *h);
int bm_rbm_sync(bm_rbm *h);

/* Variables of the TF graph by name (tf_model.py:183-202 get_tf_params; Saver
 * restore tf_model.py:22-28): "W" [V*H], "vb" [V], "hb" [H], "dW", "dvb",
 * "dhb", "q_means" [H], "sigma" [V].  n = number of floats. */
int bm_rbm_set_param(bm_rbm *h, const char *name, const float *host, size_t n);
/* the same from DEVICE memory (dense, row-major), asynchronously on the handle's stream - no host synchronisation
 * (re-initialising between runs, `init_from` another handle: base_rbm.py:668-685 without a host round trip) */
int bm_rbm_set_param_dev(bm_rbm *h, const char *name, const float *src_dev, size_t n);
/* get only, while the handle holds a tempered ensemble of M chains x R replicas (tests and tools; dense): "pt_v" [M R * V],
 * "pt_h" [M R * H], the slot partials "pt_part_v" [ceil(V/16) * M R] and "pt_part_h" [ceil(H/16) * M R], "pt_mult" [M R] */
int bm_rbm_get_param(bm_rbm *h, const char *name, float *host, size_t n);
/* device pointer of a variable / workspace for zero-copy interop (RCCL):
 * the variables above plus "grad" (fused [V*H + V + H + H] raw-sum buffer). */
int bm_rbm_dev_ptr(bm_rbm *h, const char *name, void **out_dev, size_t *out_n);

/* Replaces tf.set_random_seed(model.make_random_seed()) done by the
 * run_in_tf_session decorator on every public call (tf_model.py:20-21).
 * Sets the Philox key and resets the per-handle call counter to 0.
 * Stream convention: DESIGN.md "RNG". */
int bm_rbm_seed(bm_rbm *h, uint64_t seed);
/* global index of local row 0 (data-parallel: rank*local_batch); sample
 * bitmaps depend on the GLOBAL row so they are rank-count invariant. */
int bm_rbm_set_row_offset(bm_rbm *h, int64_t row0);

/* One CD-k update: session.run(train_op, feed_dict) at base_rbm.py:566
 * (graph: base_rbm.py:415-479).  X_dev [B, n_visible] row-major. */
int bm_rbm_train_step(bm_rbm *h, const float *X_dev, int32_t B,
                      float learning_rate, float momentum, int32_t n_gibbs_steps);
/* Same update, but the metric ops are fetched from the SAME chain in the same
 * run, as the reference does every `train_metrics_every_iter` iterations
 * (base_rbm.py:554-564).  out4 as in bm_rbm_metrics (computed before the update). */
int bm_rbm_train_step_metrics(bm_rbm *h, const float *X_dev, int32_t B,
                              float learning_rate, float momentum, int32_t n_gibbs_steps,
                              float *out4);
/* The same fetch without the host wait.  The reference only uses the MEAN of the train metrics at the end
 * of the epoch (base_rbm.py:571), so the sums of a metrics iteration are copied to a pinned ring in stream
 * order; bm_rbm_collect_metrics synchronises once and returns the pending fetches in order
 * (out4n [max_n][4], *out_n their number; at most 4096 may be pending). */
int bm_rbm_train_step_metrics_async(bm_rbm *h, const float *X_dev, int32_t B,
                                    float learning_rate, float momentum, int32_t n_gibbs_steps);
int bm_rbm_collect_metrics(bm_rbm *h, float *out4n, int32_t max_n, int32_t *out_n);
/* The `for X_batch in batch_iter(X, batch_size)` loop of _train_epoch
 * (base_rbm.py:549-571) behind ONE call: N rows, consecutive batches of `batch` rows (last one may be
 * short).  The library enqueues every update's four launches from a native loop, asynchronously on the
 * handle's stream (no synchronisation, no device-to-host traffic, one FFI crossing per run of batches);
 * the stream stays GPU-bound. */
int bm_rbm_train_epoch(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch,
                       float learning_rate, float momentum, int32_t n_gibbs_steps);

/* A snapshot of every variable that does not stop the stream (the per-epoch checkpoint of base_rbm.py:665-666 while
 * the next epoch already runs): bm_rbm_stage copies them device-to-device into slot 0 | 1 in stream order and returns;
 * bm_rbm_get_staged reads one variable of that snapshot (dense, like bm_rbm_get_param) on its own stream - it waits
 * for the staged copies only - and may be called from another host thread.  Do not re-stage a slot being read. */
int bm_rbm_stage(bm_rbm *h, int32_t slot);
int bm_rbm_get_staged(bm_rbm *h, int32_t slot, const char *name, float *host, size_t n);

/* Data-parallel split of a train step: phase 1 runs the chain and
 * leaves the raw un-normalised sums in the "grad" buffer
 * [pos-neg (V*H) | sum(X-v) (V) | sum(h0-hk) (H) | sum(hk) (H)]; the caller
 * all-reduces that buffer (RCCL) and calls phase 2 with the GLOBAL batch. */
int bm_rbm_grad_step(bm_rbm *h, const float *X_dev, int32_t B_local, int32_t n_gibbs_steps);
int bm_rbm_apply_step(bm_rbm *h, int32_t B_global, float learning_rate, float momentum);

/* transform_op.eval at base_rbm.py:697: h_means at the END of the k-step
 * chain (base_rbm.py:426,438-440).  H_dev [B, n_hidden]. */
int bm_rbm_transform(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps,
                     float *H_dev);

/* One prop-up of the handle's OWN hidden conditional (every hidden unit type) from X_dev [B, n_visible], the input taken as
 * given: no division by sigma, no dropout.  Hmean_dev / Hstate_dev [B, n_hidden] dense, either may be NULL (no states: no
 * draw).  The states are drawn at site SITE_H0 (2), step 0, with the handle's seed, call counter and row offset - what the h0
 * pass of bm_rbm_train_step draws for the same input - whatever sample_h_states says.  The call counter advances by one.
 * B <= max_batch. */
int bm_rbm_sample_h(bm_rbm *h, const float *X_dev, int32_t B, float *Hmean_dev, float *Hstate_dev);

/* The visible counterpart of bm_rbm_sample_h: one prop-down of the handle's OWN visible conditional (every visible unit type,
 * softmax groups included) from H_dev [B, n_hidden], taken as given.  Vmean_dev / Vstate_dev [B, n_visible] dense, either may
 * be NULL (no states: no draw), not both.  The states are drawn at site SITE_V (3), step 0, with the handle's seed, call counter
 * and row offset - what the first prop-down of bm_rbm_gibbs draws for the same input - whatever sample_v_states says.  The call
 * counter advances by one.  B <= max_batch. */
int bm_rbm_sample_v_from_h(bm_rbm *h, const float *H_dev, int32_t B, float *Vmean_dev, float *Vstate_dev);

/* Softmax (categorical) visible units (no counterpart in the reference): turns the visible layer of a
 * Bernoulli-visible, Bernoulli-hidden float32 handle into n_visible / K groups of K mutually exclusive units, one-hot per group;
 * K = 0 turns it off again.  bm_rbm_config is unchanged.  With l = h W^T + vb, per row and group, sequentially left to right in
 * float32: mx = max l; e[k] = exp_neg(min(mx - l[k], 80)); c[k] = c[k-1] + e[k]; S = c[K-1]; mean[k] = e[k] / S; the state is
 * the first k with c[k] > u S, u the uniform of the layer's per-element stream at the group's first unit (site and call counter
 * of a Bernoulli handle's visible pass).  The prop-up, the update and the free energy are the Bernoulli ones.  Such a handle
 * trains (train_step, _metrics, _metrics_async, _epoch), transforms, runs bm_rbm_gibbs / bm_rbm_metrics / bm_rbm_sample_h /
 * bm_rbm_sample_v_from_h / bm_rbm_free_energy(_rows) and is staged like any other; out4[1] (pll) of the metric calls is NaN,
 * out4[3] the ordinary free energy.  Refused, with a message that contains "softmax visible" and leaves the handle usable - here:
 * n_visible % K != 0, K == 1, K < 0, Gaussian visible units, Multinomial or NReLU hidden units, dbm_first / dbm_last, dropout, a
 * handle with centering, a class head, fast weights or a tempered ensemble; on such a handle: bm_rbm_ais, bm_rbm_pt_*,
 * bm_rbm_train_step_pt / _epoch_pt, bm_rbm_set_fast_weights, bm_rbm_set_centering, bm_rbm_set_classes and every bm_rbm_class_*
 * entry, bm_rbm_gibbs_clamped, bm_rbm_grad_step / _apply_step and the gradient exchange entries, bm_rbm_backprop_down /
 * _delta_update / the stack entries.  bm_rbm_set_fast_binary is accepted and runs fp32. */
int bm_rbm_set_visible_groups(bm_rbm *h, int32_t K);

/* Replicated softmax visible units (Salakhutdinov & Hinton 2009; no counterpart in the reference): turns the
 * visible layer of a Bernoulli-visible, Bernoulli-hidden float32 handle into ONE softmax over the n_visible units (2 to 16384),
 * drawn D times per row and summed into a count vector; max_length = 0 turns it off again.  Rows are count vectors: non-negative
 * integers in float32 with D_b = sum_i X[b][i] in [1, max_length], max_length < 2^24.  bm_rbm_config is unchanged.
 *   E(v, h) = -v W h - v.vb - D h.hb;   p(h_j = 1 | v) = sigmoid(D hb_j + (v W)_j), formed as z + fl(D hb_j);
 *   v | h ~ Multinomial(D, softmax(vb + W h)), means D * softmax;   F(v) = -v.vb - sum_j softplus(D hb_j + (v W)_j).
 * The softmax and the draws are multinomial_counts_kernel's (csrc/bm_rsm.h: the prefix order, draw d of global row r reads the
 * uniform at flat index r * max_length + d of the visible pass's stream).  The update is the Bernoulli one except for the hidden
 * bias, whose gradient is (1/N) sum_b D_b (h0_b - hk_b).  Where the lengths come from: the training, metric and transform chains,
 * bm_rbm_sample_h and bm_rbm_free_energy_rows compute them from their input rows; bm_rbm_sample_v_from_h and bm_rbm_gibbs take
 * them from bm_rbm_set_row_lengths.  A row that is no such count vector raises a device flag, reported once by bm_rbm_sync and
 * bm_rbm_free_energy_rows with a message that names the kind (negative entry, non-integer entry, empty row, row longer than
 * max_length).  Such a handle trains (train_step, _metrics, _metrics_async, _epoch), transforms, runs bm_rbm_metrics (out4[0] the
 * msre on counts; out4[1] pll and out4[3] are NaN), bm_rbm_sample_h and is staged like any other; always per-pass fp32 launches
 * (no chained launch; bm_rbm_set_fast_binary is accepted and runs fp32).  Refused, with a message that contains "replicated
 * softmax" and leaves the handle usable - here: max_length outside [1, 2^24), n_visible outside [2, 16384], Gaussian visible
 * units, Multinomial or NReLU hidden units, dbm_first / dbm_last, dropout, a non-zero sparsity_cost, a handle with centering, a
 * class head, fast weights, a tempered ensemble or visible groups; on such a handle: bm_rbm_free_energy (the feg metric) and every
 * entry bm_rbm_set_visible_groups lists for its handles. */
int bm_rbm_set_replicated_softmax(bm_rbm *h, int32_t max_length);

/* The lengths of the rows that the next bm_rbm_sample_v_from_h / bm_rbm_gibbs calls of a replicated-softmax handle run on:
 * D_dev [B] float32 on the device, integers in [1, max_length]; copied into the handle in stream order.  Those calls need
 * exactly B rows. */
int bm_rbm_set_row_lengths(bm_rbm *h, const float *D_dev, int32_t B);

/* Softmax visible units with incomplete rows, clamped groups and exact group conditionals.  All three entries
 * need a handle with visible groups (bm_rbm_set_visible_groups); on any other handle they are refused with a message that names
 * visible groups, and the handle stays usable.  V = G K, W [V][H].
 *
 * bm_rbm_groups_set_missing(h, on): while on, a group of an input row that is all zeros is a MISSING group: the model of that row
 * has the observed units only (shared weights).  Everything that runs the training chain - bm_rbm_train_step, _metrics,
 * _metrics_async, _epoch, bm_rbm_metrics - builds the mask of the input's empty groups first and holds those groups at zero in
 * every prop-down (visible means and states exactly 0 there); the prop-up, the update with N = B, the sparsity terms and the free
 * energy are unchanged (a zero row of v contributes nothing).  With complete rows every result equals the mode-off result bit for
 * bit.  bm_rbm_gibbs, bm_rbm_sample_v_from_h and bm_rbm_transform do not look at the mode.  Off by default;
 * bm_rbm_set_visible_groups(h, 0) turns it off.
 *
 * bm_rbm_groups_gibbs_clamped: bm_rbm_gibbs_clamped (same arguments, launches, sites, call counter, row offset; both layers always
 * sampled; Vmean_dev may be NULL) for a handle with visible groups.  clamp_mask_dev must be constant within every group - the
 * caller's guarantee, not checked: a clamped group holds clamp_val (a one-hot group, or zeros for a group that is absent), a free
 * group gets exactly the means, the uniform and the state of the unclamped pass from the same input; a clamped group's uniform is
 * consumed by position and not used.  An all-zero mask reproduces the unclamped sweep bit for bit.  B <= max_batch.
 *
 * bm_rbm_groups_scores: scores_host [B][V] (double).  For a row x whose groups are each one-hot or empty, group g with current
 * unit c (none if empty) and category k:  S[g K + k] = vb[gK+k] + sum_j softplus(a_j + W[gK+k][j]),  a_j = z_j - W[c][j] (a_j = z_j
 * for an empty group), z = x W + hb; then log p(v_g = k | v_-g) = S[gK+k] - logsumexp_k' S[gK+k'] - for an empty group the
 * posterior given the observed groups alone (the other empty groups absent).  z, a_j and the argument of the softplus are rounded
 * float32 operations, the softplus terms float32 on the hardware transcendentals (as the default AIS path), their sum and the
 * bias accumulated in double in a fixed order that depends on the shape alone.  The softmax over k is left to the caller.  B is
 * not bounded by max_batch (sliced internally); no RNG call is consumed, no parameter changes. */
int bm_rbm_groups_set_missing(bm_rbm *h, int32_t on);
int bm_rbm_groups_gibbs_clamped(bm_rbm *h, float *V_dev, float *H_dev, float *Vmean_dev, int32_t B, int32_t n_steps,
                                const float *clamp_val_dev, const float *clamp_mask_dev);
int bm_rbm_groups_scores(bm_rbm *h, const float *X_dev, int32_t B, double *scores_host);
/* AIS estimate of the log partition function of an RBM with softmax visible units, or of one of its sub-models:
 * bm_rbm_ais with a categorical base model and softmax transitions.  V = G K; O = the observed groups, observed_host [G] (0 =
 * absent; NULL: all of them).  A group outside O is absent from the model - the missing_values semantics of 3.25 - and every
 * chain state is zero there.  a = base_bias_host [V] are the base logits (NULL: a = 0, the uniform base), z = v W + hb:
 *   p_0(v) = prod_{g in O} softmax(a_g)[v_g],   log Z_0 = n_hidden log 2 + sum_{g in O} logsumexp_k a_{gK+k}   (host, double)
 *   log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta z_j),   beta_k = float32(linspace(0, 1, n_betas))[k]
 * v_0: every group in O gets one categorical draw from the logits a_g by the softmax-group rule (mx, e, sequential c, S, the first
 * k with c[k] > u S); for k = 1 .. n_betas - 1: logw += log p*_{beta_k}(v_{k-1}) - log p*_{beta_{k-1}}(v_{k-1}), then n_gibbs_steps
 * transitions h ~ Ber(sigmoid(beta_k z)), v_g ~ softmax_k(beta_k (h W^T)_{gK+k} + a + beta_k (vb - a)) for g in O and zeros
 * elsewhere - both layers always sampled; none behind the last score.  values_host [n_runs] receives logw + log Z_0 per chain.
 * RNG sites as bm_rbm_ais (Philox key = seed, counter word site + 16 t, call = beta step, row offset = chain0 + row): 7 for v_0
 * (call 0), 8 for v, 9 for h; a group's uniform is the visible layer's per-element stream read at the group's first unit, flat
 * index (chain0 + row) V + g K; an absent group's uniform is consumed by position, not used.  Chains [c, c + n) of a larger run
 * are the run of n chains at chain0 = c, bit for bit.
 * The per-beta terms are fp32 (softplus on the hardware transcendentals); the sums over the 16-column slots and over the betas
 * are DOUBLE in a fixed order: the values depend neither on the tile geometry nor on which softmax route ran (the fused SM + SA
 * flavour for groups of 2, 4, 8 or 16 in a layer of V % 4 == 0, the logits / softmax / row-dot triple for every other shape;
 * BM355_DEBUG=sm_fused=0 forces the latter).  A pattern that observes every group gives the bits of the run without a pattern.
 * Needs a handle with visible groups; refused otherwise, like the entries above.  Refused too: bad arguments (as bm_rbm_ais), a
 * pattern with no observed group.  The call draws from its own streams: it does not advance the handle's call counter, changes no
 * parameter, momentum buffer or workspace that another entry reads (the AIS workspaces are shared with bm_rbm_ais only), and does
 * not look at bm_rbm_groups_set_missing - the pattern is explicit.  Workspaces for n_runs rows are allocated on demand: max_batch
 * does not bound the number of chains. */
int bm_rbm_groups_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t n_gibbs_steps, const float *base_bias_host,
                      const uint8_t *observed_host, uint64_t seed, int64_t chain0, float *values_host);
/* Parallel tempering and the tempered negative phase over softmax visible units: bm_rbm_pt_init / _sweep / _read
 * and bm_rbm_train_step_pt / _train_epoch_pt for a handle with visible groups, under names of their own (those entries keep
 * refusing such a handle).  The contracts are theirs - the ensemble, its chain-major rows, the ladder checks, the swap step, the
 * counters, the seven steps of an update, the call counter (once per sweep or update) and the step parity (continued across calls),
 * chain0 and the chain-slice property, BM355_DEBUG=pt_sel=0 - with these differences:
 *   start      v_0 is one uniform category per group: the softmax-group rule with zero logits (e = 1, c[k] = k + 1, the first k with
 *              c[k] > u K), u the uniform at flat index ((chain0 + c) R + r) V + g K of site 11; with V0_dev [n_chains, n_visible]
 *              (complete one-hot rows: the caller's guarantee) every chain's R replicas start from its row.
 *   prop-down  v_g ~ softmax_k(l_{gK..gK+K-1}) with the logits l = fl(fl(beta_row z) + fl(beta_row vb)), z = h W^T: two rounded
 *              multiplies and one rounded add, never an FMA, so that beta_row = 1 is the plain softmax pass bit for bit; means, draw
 *              and Philox index are those of bm_rbm_set_visible_groups (site SITE_V + 16 t, the group's first unit).  One launch (the
 *              SM + SA + RT flavour of act_kernel) for groups of 2, 4, 8 or 16 in a layer of n_visible % 4 == 0, a raw pass, a groups
 *              kernel and a row-dot kernel for every other shape (BM355_DEBUG=sm_fused=0 forces the latter): the same bits.
 *   prop-up, swap   unchanged: for one-hot v the Bernoulli hidden conditional and E = -v.vb - h.hb - vWh are this model's.
 * An update takes its negative particles from the beta = 1 rows of the chains [0, B) - in the last prop-down's epilogue on the
 * one-launch route, by a gather launch on the other - and ends in the fused update of bm_rbm_train_step.
 * Refused, the handle staying usable: a handle without visible groups (the message of the entries above), a handle with
 * bm_rbm_groups_set_missing on (an ensemble row has no pattern of observed groups: not built), sweep / read / update before init,
 * B outside [1, min(max_batch, n_chains)], n_steps or n_gibbs_steps < 1, a bad ladder.  bm_rbm_set_visible_groups(h, 0) discards
 * the ensemble.  bm_rbm_train_step, bm_rbm_groups_ais and every other entry neither read nor write it.  Float32, one process. */
int bm_rbm_groups_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0);
int bm_rbm_groups_pt_sweep(bm_rbm *h, int32_t n_steps);
int bm_rbm_groups_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host);
int bm_rbm_groups_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t n_gibbs_steps);
int bm_rbm_groups_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t n_gibbs_steps);
/* Parallel tempering over replicated softmax visible units: bm_rbm_pt_* for a handle with the unit
 * (bm_rbm_set_replicated_softmax).  The tempered family over count vectors of length D is p_beta(v, h) ~ (D!/prod v_i!)
 * exp(-beta E(v, h)), E = -v W h - v.vb - D h.hb (the coefficient is the base measure, not tempered): h_j | v ~ Ber(sigmoid(beta (D hb_j
 * + (vW)_j))), v | h ~ Multinomial(D, softmax(beta (vb + W h))).  Chain c has the length lengths_host[c], an integer in [1, max_length],
 * shared by its n_temps replicas (ensemble row c * n_temps + r), so the exchange rule is bm_rbm_pt_sweep's.  V0_dev [n_chains][V]
 * (dense count rows whose sums are the lengths - checked on the device, a mismatch is refused) starts every replica of a chain at its
 * row; null: v_0 ~ Multinomial(D_c, uniform) at site 11 of the handle's seed and call counter.  A step t of a call: the prop-up at site
 * 4 + 16 t, the exchange at site 10 + 16 t, the prop-down at site 3 + 16 t, draw d of global row (chain0 + c) n_temps + r at flat index
 * row * max_length + d; the call counter and the step parity follow bm_rbm_pt_sweep: chains [chain0, chain0 + n_chains) of a larger
 * ensemble give the bits they would give there.  bm_rbm_rsm_pt_read is bm_rbm_pt_read.  bm_rbm_rsm_train_step_pt /
 * _train_epoch_pt: bm_rbm_train_step_pt / _train_epoch_pt with the negative particles of the chains [0, B); the positive rows carry
 * the batch's lengths, the negative rows the chains' lengths (the hidden-bias term of row b is D_b h0 - Dn_b hk).  bm_rbm_get_param
 * hands out "pt_v", "pt_h", "pt_part_v" [2][rows] (the float32 pair hi, lo of the double v.vb), "pt_part_h", "pt_mult" and "pt_len"
 * [rows].  The handle keeps ONE ensemble: bm_rbm_pt_init refuses a handle with the unit, bm_rbm_set_replicated_softmax refuses a
 * handle that holds a Bernoulli ensemble, bm_rbm_set_replicated_softmax(h, 0) discards a count ensemble.  Refused with an error that
 * leaves the handle usable: a handle without the unit, sweep / read / update before init, lengths outside [1, max_length], B outside
 * [1, min(max_batch, n_chains)], n_steps or n_gibbs_steps < 1, a bad ladder.  Float32, one process. */
int bm_rbm_rsm_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *lengths_host,
                       const float *V0_dev, int64_t chain0);
int bm_rbm_rsm_pt_sweep(bm_rbm *h, int32_t n_steps);
/* Launch-level probe of the tempered prop-ups of this unit (tests): h ~ Ber(sigmoid(beta (v W + D_j hb))) of the J rows of V_dev
 * [J][V] with lengths_dev [J] into H_dev [J][H], at site 4, step 0 of the handle's seed, call counter and row offset; the counter does
 * not advance.  per_row != 0: the pass of bm_rbm_rsm_pt_sweep with every row at beta (its energy partials to part_dev [ceil(H/16)][J]
 * unless null); per_row == 0: the pass of bm_rbm_rsm_ais at the launch-uniform beta.  The two give the same bits. */
int bm_debug_rsm_up(bm_rbm *h, const float *V_dev, int32_t J, const float *lengths_dev, float beta, int32_t per_row, float *H_dev,
                    float *part_dev);
int bm_rbm_rsm_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host);
int bm_rbm_rsm_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t n_gibbs_steps);
int bm_rbm_rsm_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t n_gibbs_steps);
/* AIS estimates of the log partition functions of an RBM with replicated softmax visible units.  The partition
 * function depends on the document length, Z_D = sum_h exp(D h.hb) (sum_i exp(vb_i + (W h)_i))^D, so every chain has a length of
 * its own: row r is ONE chain over count vectors of lengths_host[r] tokens, an integer in [1, max_length]; chains of different
 * lengths run side by side in the same launches.  a = base_logits_host [V] (NULL: a = 0, the uniform base), t = D hb + v W:
 *   p_0(v) = Multinomial(D, softmax(a)),   log Z_0(D) = n_hidden log 2 + D logsumexp(a)   (host, double)
 *   log p*_beta(v) = log(D! / prod v_i!) + (1 - beta) a.v + beta vb.v + sum_j softplus(beta t_j),  beta_k = float32(linspace(0, 1, n_betas))[k]
 * v_0 ~ p_0; for k = 1 .. n_betas - 1: logw += (beta_k - beta_{k-1}) v.(vb - a) + sum_j [softplus(beta_k t_j) - softplus(beta_{k-1} t_j)]
 * (the coefficient cancels), then n_gibbs_steps transitions h ~ Ber(sigmoid(beta_k t)), v ~ Multinomial(D, softmax(a + beta_k (vb - a)
 * + beta_k W h)) - both layers always sampled; none behind the last score.  values_host [n_rows] receives logw + log Z_0(D_r).
 * The hidden pass forms x = fl(beta fl(z + fl(D hb_j))), three rounded steps; the counts are multinomial_counts_kernel's (csrc/bm_rsm.h:
 * the prefix order).  RNG sites as bm_rbm_ais (Philox key = seed, counter word site + 16 t, call = beta step): 7 for v_0 (call 0), 8
 * for v, 9 for h; draw d of row r reads the uniform at flat index (chain0 + r) max_length + d of the visible pass's stream, hidden unit
 * j the one at (chain0 + r) n_hidden + j.  Rows [c, c + n) of a larger run are the run of those n lengths at chain0 = c, bit for bit.
 * The per-beta softplus terms are fp32 (hardware transcendentals); v.(vb - a) is summed in DOUBLE from the counts (every product
 * exact) and handed to the score as a float32 pair (hi, lo), exact to 2^-48 of its value; the sums over the slots and over the betas
 * are double in a fixed order.  Needs a handle with replicated softmax visible units; refused otherwise, and for bad arguments
 * (n_betas < 2, n_rows or n_gibbs_steps < 1, chain0 < 0, a length that is no integer in [1, max_length], null pointers), with a
 * message that names bm_rbm_rsm_ais, before anything is enqueued; the handle stays usable.  The call draws from its own streams: it
 * does not advance the handle's call counter, changes no parameter or momentum buffer, and touches no workspace that another entry
 * reads - the lengths of bm_rbm_set_row_lengths and of the last batch included (the AIS workspaces are shared with bm_rbm_ais
 * only).  Workspaces for n_rows rows are allocated on demand: max_batch does not bound the number of chains. */
int bm_rbm_rsm_ais(bm_rbm *h, int32_t n_betas, int32_t n_rows, int32_t n_gibbs_steps, const float *base_logits_host,
                   const float *lengths_host, uint64_t seed, int64_t chain0, float *values_host);

/* Gaussian visible units as ONE joint model (no counterpart in the reference): AIS log Z, per-row free energies and
 * parallel tempering for a float32 handle with Gaussian visible and Bernoulli hidden units, under names of their own - bm_rbm_ais,
 * bm_rbm_free_energy_rows and bm_rbm_pt_* keep refusing such a handle.  The model is the joint over the scaled variable u = x / sigma
 * whose conditionals are the reference's free energy and prop-down, c_i = fl32(vb_i / sigma_i):
 *   E(u, h) = 1/2 |u - c|^2 - u W h - hb.h;   h | u ~ Ber(sigmoid(u W + hb));   u | h ~ N(c + W h, I);   x = sigma u.
 * (The training chain of bm_rbm_train_step feeds UNSCALED samples back into its prop-up, as the reference does: for sigma != 1 that is
 * the Gibbs sampler of no joint; these entries use the sampler above.  With sigma = 1 the two coincide.)  Everything runs on u; data
 * units appear only as u = fl32(x / sigma) on the way in and x = fl32(u sigma) on the way out.  Always per-pass fp32 launches.
 *
 * bm_rbm_gauss_ais: bm_rbm_ais with the base model p_0(u) = N(a, I), h uniform; a = base_mean_host [n_visible] in the SCALED variable
 * (NULL: a = 0).  beta_k = float32(linspace(0, 1, n_betas))[k],
 *   log p*_beta(u) = -(1 - beta) 1/2 |u - a|^2 - beta 1/2 |u - c|^2 + sum_j softplus(beta (u W + hb)_j),
 *   log Z_0 = (V/2) log 2 pi + H log 2 + sum_i log sigma_i + 1/2 (|a|^2 - |c|^2)      (host, double; the last term: see below)
 * u_0 = a + n; for k = 1 .. n_betas - 1: logw += (beta_k - beta_{k-1}) u.(c - a) + sum_j [softplus(beta_k z_j) - softplus(beta_{k-1} z_j)],
 * then n_gibbs_steps transitions h ~ Ber(sigmoid(beta_k (u W + hb))), u ~ N(a + beta_k (c - a) + beta_k W h, I); none behind the last
 * score.  The score's visible term is (beta_k - beta_{k-1}) [u.(c - a) + 1/2 (|a|^2 - |c|^2)]: its constant sums to 1/2 (|a|^2 - |c|^2)
 * over the path and is carried by log Z_0.  values_host [n_runs] receives logw + log Z_0: estimates of the log normaliser of
 * exp(-F(x / sigma)) over x (data units: sum log sigma included).  RNG sites, call = beta step, chain0 and the chain-slice property as
 * bm_rbm_ais; a normal draw is the one of the flat index (chain0 + r) n_visible + i under the Gaussian layer's word-to-draw mapping.
 * The states are float32 and reproducible bit for bit; the log-weights are double sums of float32 partials.
 *
 * bm_rbm_gauss_free_energy_rows: F(x / sigma) = 1/2 |u - c|^2 - sum_j softplus((u W + hb)_j) of X_dev [B, n_visible] (data units) into
 * out_host [B] DOUBLE; B is not bounded by max_batch; no dropout, no RNG call consumed.  log density(x) = -F - log Z.
 *
 * bm_rbm_gauss_pt_init / _sweep / _read: bm_rbm_pt_* on an ensemble of its own (bm_rbm_pt_* never see it).  The contracts are theirs -
 * chain-major rows, the ladder checks, the swap step and its counters, the call counter (once per sweep), the step parity, chain0 and
 * the chain-slice property - with these differences:
 *   start      u_0 = fl(c + fl(n sd_r)), n the normal at flat index ((chain0 + c) R + r) V + i of site 11, or, with V0_dev [n_chains,
 *              n_visible] in DATA units, u_0 = fl32(V0 / sigma) for all R replicas of a chain.
 *   prop-down  u ~ N(c + W h, I / beta_row): m = fl(z + c), s = fl(m + fl(n sd[idx_row])), sd[r] = float32(1 / sqrt(double(beta_r))),
 *              exactly 1 at beta = 1: the temperature changes the VARIANCE, not the mean.  One launch (the RT + GT flavour of
 *              act_kernel) that also leaves the slot partials of -1/2 (s - c)^2 from its registers; BM355_DEBUG=gt_fused=0: a raw pass
 *              and a row kernel, the same bits.
 *   swap       unchanged: with those partials and the prop-up's h.(u W + hb), E = 1/2 |u - c|^2 - h.(u W + hb).
 *   read       V_dev receives x = fl32(u sigma) of the beta = 1 rows.
 * The centre c is the one of the parameters at init.  Refused, the handle staying usable, with a message that names the entry: a handle
 * whose visible units are not Gaussian, Multinomial or NReLU hidden units, dbm_first / dbm_last, null pointers, bad AIS arguments, a bad
 * ladder, n_steps < 1, sweep / read before init.  None of the entries changes a parameter or a momentum buffer; AIS and the free
 * energies do not advance the call counter.  Float32, one process. */
int bm_rbm_gauss_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t n_gibbs_steps, const float *base_mean_host, uint64_t seed,
                     int64_t chain0, float *values_host);
int bm_rbm_gauss_free_energy_rows(bm_rbm *h, const float *X_dev, int32_t B, double *out_host);
int bm_rbm_gauss_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0);
int bm_rbm_gauss_pt_sweep(bm_rbm *h, int32_t n_steps);
int bm_rbm_gauss_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host);

/* Metric fetches of base_rbm.py:554-564,578,605,612: out[0]=msre (:486-488),
 * out[1]=pll (:496-513), out[2]=l2_loss (:482-484), out[3]=free_energy
 * (:516-517; rbm.py:17-22 / :109-116).  Runs the same chain as train_step
 * without updating parameters.  `out` is host memory (4 floats). */
int bm_rbm_metrics(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps,
                   float *out4);
/* batch-mean free energy only (free_energy_op, base_rbm.py:516-517). */
int bm_rbm_free_energy(bm_rbm *h, const float *X_dev, int32_t B, float *out1);
/* Per-row free energies F(x) = -x.vb - sum_j softplus((x W + hb)_j) of X_dev [B, n_visible] into out_host [B]: the
 * RBM's own parameters, no dropout, no multiplier, no RNG call consumed; B is not bounded by max_batch.  log p(x) =
 * -F(x) - log Z.  The softplus terms are the slot partials of one prop-up (ActArgs::rowacc_single); a row kernel adds them
 * and x.vb in double.  Bernoulli-Bernoulli handles without dbm_first / dbm_last only (as bm_rbm_ais). */
int bm_rbm_free_energy_rows(bm_rbm *h, const float *X_dev, int32_t B, float *out_host);
/* AIS estimate of the RBM's OWN log partition function (no counterpart in the reference, whose only AIS is the DBM's;
 * Salakhutdinov & Murray 2008): n_runs chains from the base-rate model p_0(v) ~ exp(a.v), a = base_bias_host [n_visible]
 * (NULL: a = 0, the uniform base), through beta_k = linspace(0, 1, n_betas)[k], the hidden layer summed out:
 *   log p*_beta(v) = (1 - beta) a.v + beta vb.v + sum_j softplus(beta (v W + hb)_j),  log Z_0 = n_hidden log 2 + sum_i softplus(a_i).
 * v_0 ~ Ber(sigmoid(a)); for k = 1 .. n_betas - 1: logw += log p*_{beta_k}(v_{k-1}) - log p*_{beta_{k-1}}(v_{k-1}), then
 * n_gibbs_steps transitions h ~ Ber(sigmoid(beta_k (v W + hb))), v ~ Ber(sigmoid(beta_k (h W^T + vb) + (1 - beta_k) a)) - both
 * layers always sampled, whatever sample_v_states / sample_h_states say; none behind the last score.  values_host [n_runs]
 * receives logw + log Z_0 per chain (log_mean_exp and the error bars stay with the caller).  No dropout.
 * The chain workspaces are allocated for n_runs rows on demand: max_batch does not bound the number of chains.
 * RNG sites (Philox key = seed, counter word site + 16 t with t the Gibbs step, call = beta step k, row offset = chain0 +
 * row, the global chain index): 7 for v_0 (call 0), 8 for v, 9 for h.  Chains [c, c + n) of a larger run are therefore the
 * run of n chains at chain0 = c, bit for bit.
 * The per-beta terms are fp32; their sums over the 16-column slots and over the betas are kept in DOUBLE in a fixed order
 * (as bm_dbm_ais): the values do not depend on the tile geometry and do not vary from run to run.  Between the upload of
 * a / the betas and the download of the values the host only enqueues launches: per beta step 2 n_gibbs_steps propagation
 * launches and one score launch.  Fast-binary mode does not apply: the fp32 path runs, the default's bits.
 * Refused: Gaussian visible units, Multinomial hidden units, dbm_first / dbm_last handles (their conditionals belong to no
 * single joint distribution). */
int bm_rbm_ais(bm_rbm *h, int32_t n_betas, int32_t n_runs, int32_t n_gibbs_steps, const float *base_bias_host,
               uint64_t seed, int64_t chain0, float *values_host);

/* Pure block-Gibbs sampling sweep (R5/R6 of SURVEY §8a; base_rbm.py:367-413):
 * n_steps of h->v->h starting from hidden states H_dev [B, n_hidden] (in/out);
 * V_dev [B, n_visible] receives the last visible states.  No parameter update. */
int bm_rbm_gibbs(bm_rbm *h, float *H_dev, float *V_dev, int32_t B, int32_t n_steps);

/* Conditional sampling: block-Gibbs with CLAMPED visible units.  All pointers are device pointers, dense
 * [B, n_visible] / [B, n_hidden]; a visible unit of a row is clamped (observed) where clamp_mask_dev is non-zero and then
 * holds clamp_val_dev (any float: {0,1}, grey levels, reals for Gaussian visibles - already divided by sigma, as the chain
 * of bm_rbm_train_step sees its input).
 * V_dev is in/out: the initial visible states; its clamped entries are overwritten from clamp_val_dev first.  Then, for
 * t = 0 .. n_steps-1:  h ~ p(h|v) at site SITE_H + 16 t,  v ~ p(v|h) at site SITE_V + 16 t with the clamp applied in that
 * pass's epilogue.  A clamped output's random words are skipped by position: the free entries get the bits an unclamped
 * sweep from the same states would give them.  Both layers are always sampled (the handle's sample_*_states flags do not
 * apply); the dbm_first / dbm_last multipliers do.  V_dev and H_dev receive the last states, Vmean_dev (may be NULL) the
 * last visible pass's means - clamped entries hold the clamp value in both.  The call counter advances once; no parameter,
 * momentum buffer or workspace another entry point reads is changed.  Always per-pass fp32 launches: BM355_DEBUG=chain= and
 * fast-binary mode do not change its bits.  Row r draws as global row (row offset + r): a slice of rows with
 * bm_rbm_set_row_offset reproduces those rows of the whole.
 * Errors: B outside [1, max_batch], n_steps < 1, Multinomial hidden units.  (No float64 counterpart.) */
int bm_rbm_gibbs_clamped(bm_rbm *h, float *V_dev, float *H_dev, float *Vmean_dev, int32_t B, int32_t n_steps,
                         const float *clamp_val_dev, const float *clamp_mask_dev);

/* Parallel tempering (replica exchange; Desjardins et al. 2010, Cho et al. 2010): unconditional samples of a
 * trained RBM that mix between modes.  The tempered family is p_beta(v, h) ~ exp(-beta E(v, h)), E = -v.vb - h.hb - vWh, on a
 * ladder betas[0] < ... < betas[R-1] = 1.  An ensemble of n_chains independent chains with R = n_temps replicas each lives in
 * the handle: rows are chain-major (row c R + r is slot r of chain c; a slot starts at ladder index r), allocated on demand -
 * max_batch does not bound it - and freed with the handle.  Every replica of every chain takes part in ONE launch per pass,
 * each row at its own temperature (the RT flavour of act_kernel, ActArgs::row_mult).
 *   bm_rbm_pt_init   builds the ensemble: v_0 ~ Ber(1/2) (site 11, the handle's current call) or, with V0_dev [n_chains,
 *                    n_visible] (device, dense), every chain's R replicas start from its row of V0_dev.  Resets the swap counters
 *                    and the step parity.  Does not advance the call counter.
 *   bm_rbm_pt_sweep  n_steps steps; step t: h ~ p_beta(h | v) for every row (site SITE_H + 16 t), leaving h.(vW + hb) as slot
 *                    partials; the swap step; v ~ p_beta(v | h) (site SITE_V + 16 t), leaving v.vb.  The swap step proposes,
 *                    per chain, to exchange the replicas at ladder indices (p, p + 1) for the even p when the global step number
 *                    (counted from bm_rbm_pt_init, across calls) is even, for the odd p otherwise:
 *                    delta = (beta_p - beta_{p+1})(E_p - E_{p+1}) in double from the float32 slot partials added in ascending
 *                    order; accepted iff delta >= 0 or u < exp(delta), u the uniform at flat index (chain0 + c)(R - 1) + p of
 *                    site 10 + 16 t.  An accepted swap exchanges the two rows' temperatures and ladder indices; states stay in
 *                    place.  The call counter advances once per bm_rbm_pt_sweep.
 *   bm_rbm_pt_read   copies, for every chain, the row at beta = 1 to V_dev [n_chains, n_visible] (NULL: nothing is copied) and
 *                    its hidden states - the ones that row's v was drawn from - to H_dev [n_chains, n_hidden] (NULL ok);
 *                    swaps_host [2][R-1] (NULL ok) receives attempts, then accepts, per ladder pair since bm_rbm_pt_init;
 *                    ladder_idx_host [n_chains R] (NULL ok) the ladder index of every row.  Waits for the stream.
 * The global row of the RNG streams is (chain0 + c) R + r: chains [c, c + n) of a larger ensemble are the ensemble of n chains
 * at chain0 = c, bit for bit.  Always per-pass fp32 launches (as bm_rbm_ais): BM355_DEBUG=chain= and fast-binary mode do not
 * change the bits.  With n_temps = 1 a sweep from V0 equals bm_rbm_gibbs_clamped with an all-zero mask from the same V0, seed
 * and call, bit for bit.  No parameter, momentum buffer or workspace another entry point reads is touched.
 * Errors: n_temps < 1, n_chains < 1, betas not strictly increasing inside (0, 1] or betas[R-1] != 1, sweep or read before
 * init, n_steps < 1, and the refusals of bm_rbm_ais (Gaussian visible units, Multinomial hidden units, dbm_first / dbm_last). */
int bm_rbm_pt_init(bm_rbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0);
int bm_rbm_pt_sweep(bm_rbm *h, int32_t n_steps);
int bm_rbm_pt_read(bm_rbm *h, float *V_dev, float *H_dev, int64_t *swaps_host, int32_t *ladder_idx_host);

/* Tempered negative phase: one CD-style update whose negative particles are the beta = 1 rows of the
 * ensemble bm_rbm_pt_init built, instead of a chain started at the batch.  On the handle's stream, no host synchronisation:
 *   1. the v.vb slot partials of every ensemble row are recomputed from its state and the CURRENT vb (the previous update
 *      changed vb after the prop-down that left them; with an unchanged vb this rewrites the same bits);
 *   2. positive phase: the means E[h | x] of the batch (nothing is drawn);
 *   3. n_gibbs_steps steps of bm_rbm_pt_sweep on all n_chains R rows (sites SITE_H + 16 t, 10 + 16 t, SITE_V + 16 t of the
 *      handle's call counter; the swap parity continues the ensemble's step count);
 *   4. the last prop-down also leaves the beta = 1 row of every chain c < B as negative particle c (in its epilogue;
 *      BM355_DEBUG=pt_sel=0: by a gather launch - the same bits);
 *   5. negative phase: the means E[h | particle];
 *   6. the fused update of bm_rbm_train_step (momentum, l2, sparsity, q_means) on these statistics.
 * The call counter advances once per update, the ensemble's step count by n_gibbs_steps.  A batch shorter than n_chains
 * uses the chains [0, B); every row still sweeps.
 * bm_rbm_train_epoch_pt is the native batch loop: the launches and call counters of one bm_rbm_train_step_pt per batch of
 * `batch` rows (the last batch may be short).
 * Errors: no ensemble, B outside [1, min(max_batch, n_chains)], n_gibbs_steps < 1, a handle with dropout, a momentum buffer
 * sharded by bm_rbm_exchange_apply_direct (as bm_rbm_train_step).  Float32, one process. */
int bm_rbm_train_step_pt(bm_rbm *h, const float *X_dev, int32_t B, float lr, float mom, int32_t n_gibbs_steps);
int bm_rbm_train_epoch_pt(bm_rbm *h, const float *X_dev, int64_t N, int32_t batch, float lr, float mom, int32_t n_gibbs_steps);

/* ---- Fast-weights PCD (FPCD, Tieleman & Hinton 2009) ---------------------------------------------------
 * A second, quickly decaying parameter set Wf [V][H], vbf [V], hbf [H] (float32) that learns from the gradient of every
 * tempered update at its own rate.  While the mode is on, bm_rbm_train_step_pt / _train_epoch_pt run their whole negative
 * phase - the v.vb rescore, the n_gibbs_steps tempered steps of all rows with their swap energies, the negative means of the
 * selected rows - under the effective set We = W + Wf, vbe = vb + vbf, hbe = hb + hbf (one float32 addition per element); the
 * positive phase and the regular update (momentum, l2, sparsity, q_means) are exactly those of the mode off.  In the update's
 * launches, with g0 the gradient the regular rule starts from (raw / N, before l2 and penalty; biases: the column sums / N)
 * and every product and sum rounded once:
 *   f <- fast_decay * f + fast_learning_rate * g0;      effective <- regular_new + f
 * No random number is drawn for it: an update with fast weights draws what the plain tempered update draws.  With one
 * temperature this is FPCD proper; with more, the whole ladder runs under the effective set.  Nothing else reads the fast or
 * effective parameters: bm_rbm_pt_sweep, sampling, the metrics, transform, AIS, the class head and the CD updates see the
 * regular model.  Any other writer of W, vb or hb (bm_rbm_set_param[_dev], the CD updates, bm_rbm_apply_step, the exchanges)
 * leaves the effective copies stale; the next tempered update or read of them rebuilds them first, so such calls between two
 * fast-weights updates are legal.
 * on = 1 from off: allocates the sets and starts from a zero fast set; on = 1 while on: only changes the two scalars;
 * on = 0: releases the sets (the scalars are not read) - the handle is then what it was before.
 * Variables of bm_rbm_set_param / get_param while the mode is on: "W_fast", "vb_fast", "hb_fast" (get and set), "W_eff",
 * "vb_eff", "hb_eff" (get only).
 * Refused (the error names fast weights): what bm_rbm_pt_init refuses, a handle with dropout, a centred handle - and
 * bm_rbm_set_centering(on) while fast weights are on -, fast_learning_rate negative or not finite, fast_decay outside
 * [0, 1).  Float32 only; not combined with the class head's training, the DBM or data parallelism (none of them reads it). */
int bm_rbm_set_fast_weights(bm_rbm *h, int32_t on, float fast_learning_rate, float fast_decay);

/* the handle's hipStream_t (as void*), so a host can enqueue collectives on
 * the same stream (torch.cuda.ExternalStream) without host synchronisation. */
int bm_rbm_stream(bm_rbm *h, void **out_stream);

/* Per-kernel-class HIP-event timing (bench.py roofline leg).  While enabled,
 * every launch is bracketed by events on the handle's stream;
 * bm_rbm_kernel_times() synchronises and returns, for class c in
 * {0: prop-up act_kernel, 1: prop-down act_kernel, 2: grad_kernel,
 *  3: colsum_kernel, 4: bias/apply kernels, 5: other}, the summed duration
 * ms[c] and the launch count n[c] since the last enable. */
#define BM_NUM_KERNEL_CLASSES 6
int bm_rbm_profile(bm_rbm *h, int32_t enable);
int bm_rbm_kernel_times(bm_rbm *h, float *ms6, int32_t *n6);

/* Chained launches (csrc/bm_chain.h): h0 and the k Gibbs steps of base_rbm.py:417-426 / the sweeps of bm_rbm_gibbs run as
 * ONE launch where the shape allows it (BM355_DEBUG=chain=0: never, 1: default rule, 2: wherever legal).  out3 = {chained
 * launches issued so far, tiles they must compute, mode}; bm_rbm_sync reports a launch that did not complete as an error. */
int bm_rbm_chain_stats(bm_rbm *h, int64_t *out3);

/* HIP-event timer on the handle's stream (bench.py roofline leg). */
int bm_rbm_timer_start(bm_rbm *h);
int bm_rbm_timer_stop(bm_rbm *h, float *out_ms);
int bm_rbm_timer_mark(bm_rbm *h);                       /* record the end event only (no host wait) ... */
int bm_rbm_timer_elapsed(bm_rbm *h, float *out_ms);     /* ... wait for it and read start -> mark */

/* ---- float64 RBM path ---------------------------------------------------------------------
 * The reference's dtype is a constructor argument (base/mixin.py:15, DtypeMixin) and its own
 * tests train a float64 BernoulliRBM (rbm/tests/test_rbm.py:53-56,70-73).  Same fetch sites as
 * the float32 entry points above, every buffer and scalar in double; Bernoulli or Gaussian visible units,
 * Bernoulli or Multinomial hidden units.  Variables as in
 * bm_rbm_set_param.  Compatibility path on the FP64 matrix cores, ~3x the float32 update. */
typedef struct bm_rbm64 bm_rbm64;
/* hyper5 = {l2, sparsity_target, sparsity_cost, sparsity_damping, dropout (<0: off)} as doubles (a Python
 * float is a double; the float fields of cfg would round them); NULL: take them from cfg */
int bm_rbm64_create(const bm_rbm_config *cfg, const double *hyper5, bm_rbm64 **out);
/* The width limit of a Multinomial hidden layer, float32 (RBM and DBM) and float64: the softmax stages a row in DYNAMIC LDS
 * (two reals per unit), so the limit is what the runtime allows one workgroup of that kernel, capped at 8192.  A query, no
 * launch: out4 = {hipDeviceAttributeMaxSharedMemoryPerBlock, the kernel's static LDS bytes, the dynamic LDS bytes a launch of
 * it may ask for, the largest n_hidden the create calls accept}. */
int bm_rbm_multinomial_limit(int64_t *out4);
int bm_rbm64_multinomial_limit(int64_t *out4);
int bm_rbm64_destroy(bm_rbm64 *h);
int bm_rbm64_sync(bm_rbm64 *h);
int bm_rbm64_seed(bm_rbm64 *h, uint64_t seed);                                  /* tf_model.py:20-21 */
int bm_rbm64_set_row_offset(bm_rbm64 *h, int64_t row0);
int bm_rbm64_set_param(bm_rbm64 *h, const char *name, const double *host, size_t n);   /* tf_model.py:22-28 */
int bm_rbm64_get_param(bm_rbm64 *h, const char *name, double *host, size_t n);         /* tf_model.py:183-202 */
int bm_rbm64_train_step(bm_rbm64 *h, const double *X_dev, int32_t B,                    /* base_rbm.py:566 */
                        double learning_rate, double momentum, int32_t n_gibbs_steps);
int bm_rbm64_train_step_metrics(bm_rbm64 *h, const double *X_dev, int32_t B,            /* base_rbm.py:554-564 */
                                double learning_rate, double momentum, int32_t n_gibbs_steps, double *out4);
int bm_rbm64_transform(bm_rbm64 *h, const double *X_dev, int32_t B, int32_t n_gibbs_steps,   /* base_rbm.py:697 */
                       double *H_dev);
int bm_rbm64_metrics(bm_rbm64 *h, const double *X_dev, int32_t B, int32_t n_gibbs_steps,     /* base_rbm.py:578 */
                     double *out4);
int bm_rbm64_free_energy(bm_rbm64 *h, const double *X_dev, int32_t B, double *out1);          /* base_rbm.py:605,612 */


/* ------------------------------------------------------------------- DBM */
typedef struct bm_dbm bm_dbm;

#define BM_DBM_MAX_LAYERS 4

/* ctor kwargs of DBM.__init__ (dbm.py:89-99) + layer sizes (dbm.py:207-231). */
typedef struct bm_dbm_config {
    int32_t n_layers;                       /* number of hidden layers */
    int32_t n_visible;
    int32_t n_hiddens[BM_DBM_MAX_LAYERS];
    int32_t v_unit;                         /* BM_UNIT_* of the visible layer */
    int32_t sample_v_states;
    int32_t sample_h_states[BM_DBM_MAX_LAYERS];
    int32_t n_particles;                    /* M (dbm.py:254-255) */
    int32_t batch_size;                     /* N; mu variables are [batch_size, n_i] (dbm.py:345-348) */
    int32_t max_mf_updates;
    float   mf_tol;
    float   l2;
    float   max_norm;                       /* +inf => off (dbm.py:511-513) */
    float   sparsity_target[BM_DBM_MAX_LAYERS];
    float   sparsity_cost[BM_DBM_MAX_LAYERS];
    float   sparsity_damping;
    /* hidden layer kinds (layers.py:39-70; the CIFAR DBM of examples/dbm_cifar.py is Gaussian-Bernoulli-
     * Multinomial): BM_UNIT_BERNOULLI (0, default) or BM_UNIT_MULTINOMIAL with n_samples[i] draws per row */
    int32_t h_unit[BM_DBM_MAX_LAYERS];
    int32_t n_samples[BM_DBM_MAX_LAYERS];
} bm_dbm_config;

int bm_dbm_create(const bm_dbm_config *cfg, bm_dbm **out);
int bm_dbm_destroy(bm_dbm *h);
int bm_dbm_sync(bm_dbm *h);
int bm_dbm_seed(bm_dbm *h, uint64_t seed);
int bm_dbm_set_row_offset(bm_dbm *h, int64_t row0, int64_t particle0);

/* names: "W","W_1",.. "hb","hb_1",.. "vb", "dW*","dhb*","dvb", "mu*","q_means*",
 * "mu_means*", "v" (particles [M,V]), "h","h_1",.. ([M,n_i]), "sigma"
 * (get_tf_params naming, examples/dbm_mnist.py:367-371). */
int bm_dbm_set_param(bm_dbm *h, const char *name, const float *host, size_t n);
int bm_dbm_get_param(bm_dbm *h, const char *name, float *host, size_t n);
int bm_dbm_dev_ptr(bm_dbm *h, const char *name, void **out_dev, size_t *out_n);

/* session.run(train_op) at dbm.py:805 (graph dbm.py:515-621): mean-field on
 * X_dev [batch_size, V], n_gibbs_steps PCD sweeps on the particles, gradient
 * + sparsity + momentum + max-norm update.  out_n_mf (host, may be NULL)
 * receives the executed mean-field sweeps (n_mf_updates, dbm.py:631);
 * out_msre (host, may be NULL) the reconstruction msre (dbm.py:625-630). */
int bm_dbm_train_step(bm_dbm *h, const float *X_dev, float learning_rate, float momentum,
                      int32_t n_gibbs_steps, int32_t *out_n_mf, float *out_msre);
/* session.run([msre, n_mf_updates]) at dbm.py:813 (_run_val_metrics): the two tensors are built under
 * control dependencies on the mean-field AND the particle updates (dbm.py:521-523), so this fetch runs
 * the mean-field on X_dev, advances the fantasy particles by n_gibbs_steps, and returns the
 * reconstruction msre (dbm.py:625-630); no parameter update. */
int bm_dbm_metrics(bm_dbm *h, const float *X_dev, int32_t n_gibbs_steps, int32_t *out_n_mf, float *out_msre);
/* data-parallel halves, as for the RBM: phase 1 (mean-field, PCD, raw sums) leaves
 * [sum_b below^T mu_i | sum_m below^T H_i per layer | column sums of X, v, mu_i, H_i] in the
 * "grad" buffer (bm_dbm_dev_ptr); the caller all-reduces it; phase 2 applies the update of
 * dbm.py:550-621 with the GLOBAL batch size and particle count. */
int bm_dbm_grad_step(bm_dbm *h, const float *X_dev, int32_t n_gibbs_steps, int32_t *out_n_mf);
int bm_dbm_apply_step(bm_dbm *h, int32_t N_global, int32_t M_global,
                      float learning_rate, float momentum);
/* The mean-field loop condition (dbm.py:449-452) is a max over ALL rows of the minibatch:
 * under data parallelism the library calls `fn(local_max, ctx)` once per sweep and uses the
 * returned value (the caller implements it as an all-reduce(max) over ranks).  NULL = local. */
int bm_dbm_set_mf_allreduce(bm_dbm *h, float (*fn)(float local_max, void *ctx), void *ctx);
int bm_dbm_stream(bm_dbm *h, void **out_stream);

/* _make_mf (dbm.py:429-478) on X_dev [batch_size, V]; leaves mu in the
 * handle; copies the top layer's mu to MU_top_dev if non-NULL
 * (transform, dbm.py:859-872). */
int bm_dbm_mean_field(bm_dbm *h, const float *X_dev, float *MU_top_dev, int32_t *out_n_mf);
/* reconstruction op (dbm.py:625-633, public dbm.py:874-885): runs MF then
 * sigma(mu0 W0^T + vb) into R_dev [batch_size, V]. */
int bm_dbm_reconstruct(bm_dbm *h, const float *X_dev, float *R_dev);
/* sample_v op (dbm.py:641-648, public :887-897): k PCD sweeps, one mean
 * sweep, v <- v_means; copies v to V_dev [M, V] if non-NULL. */
int bm_dbm_sample_v(bm_dbm *h, int32_t n_gibbs_steps, float *V_dev);
/* bm_dbm_sample_v with clamped visible units: clamp_val_dev / clamp_mask_dev are dense device arrays
 * [M, V]; where the mask is non-zero the visible unit of that particle holds the clamp value.  The visible layer of the
 * persistent particles is overwritten at the clamped entries before the first sweep, and every visible-layer pass of the
 * call - the n_gibbs_steps sampled sweeps and the n_gibbs_steps mean sweeps behind them - applies the clamp in its epilogue.
 * Sites, the call counter and the effect on the particles are those of bm_dbm_sample_v; with an all-zero mask the two calls
 * are bit-identical.  n_gibbs_steps == 0: no sweep runs, the clamp alone is applied.  Visible units Bernoulli or Gaussian
 * (clamp values in the engine's units); always fp32 launches, whatever bm_dbm_set_fast_binary says.
 * Errors: n_gibbs_steps < 0, null clamp pointers, a Multinomial hidden layer.  (No float64 counterpart.) */
int bm_dbm_sample_v_clamped(bm_dbm *h, int32_t n_gibbs_steps, const float *clamp_val_dev, const float *clamp_mask_dev,
                            float *V_dev);
/* Parallel tempering of a DBM (replica exchange), the counterpart of bm_rbm_pt_*: n_chains independent chains,
 * each with one replica per temperature of the ladder 0 < betas[0] < ... < betas[n_temps-1] = 1 of the family
 *   p_beta(v, h1, h2) ~ exp(-beta E),  -E = v.vb + h1.b1 + h2.b2 + v W0 h1 + h1 W1 h2
 * on the handle's own parameters, for stacks of ONE or TWO Bernoulli hidden layers over Bernoulli visible units (float32).  The
 * ensemble lives in the handle: rows are chain-major (row c R + r is slot r of chain c; a slot starts at ladder index r),
 * allocated on demand - neither batch_size nor n_particles bounds it - and freed with the handle.
 *   bm_dbm_pt_init   builds the ensemble: v_0 ~ Ber(1/2) (site 15 of the handle's current call) or, with V0_dev [n_chains,
 *                    n_visible] (device, dense), every chain's R replicas start from its row of V0_dev; h2_0 ~ Ber(1/2) always
 *                    (site 15 + 16).  Resets the swap counters and the step parity.  Does not advance the call counter.
 *   bm_dbm_pt_sweep  n_steps steps in the order of a Gibbs sweep, every layer sampled; step t: h1 ~ p_beta(h1 | v, h2) for every
 *                    row (site 8 + 16 t; one launch of two K segments), leaving h1.(v W0 + h2 W1^T + b1) as slot partials; the
 *                    swap step; h2 ~ p_beta(h2 | h1) (site 9 + 16 t), leaving h2.b2; v ~ p_beta(v | h1) (site 12 + 16 t),
 *                    leaving v.vb.  At the swap the state of a row is (v_t, h1_{t+1}, h2_t) and the three partial arrays are its
 *                    -E: per row the v.vb slots, then the h2.b2 slots, then the h1 slots are added in ascending order in double.
 *                    Pairing, parity (global step number since the init, across calls), acceptance rule and counters are those
 *                    of bm_rbm_pt_sweep; the uniform of chain c, pair p is the one at flat index (chain0 + c)(R - 1) + p of site
 *                    14 + 16 t.  The call counter advances once per bm_dbm_pt_sweep.
 *   bm_dbm_pt_read   copies, for every chain, the row at beta = 1 to V_dev [n_chains, n_visible] (NULL: nothing is copied), its
 *                    h1 to H1_dev [n_chains, n_1] (NULL ok; needs V_dev) and its h2 to H2_dev [n_chains, n_2] (NULL ok; two-layer
 *                    stacks only); swaps_host [2][R-1] (NULL ok) receives attempts, then accepts, per ladder pair since the init;
 *                    ladder_idx_host [n_chains R] (NULL ok) the ladder index of every row.  Waits for the stream.
 * The global row of the RNG streams is (chain0 + c) R + r: chains [c, c + n) of a larger ensemble are the ensemble of n chains
 * at chain0 = c, bit for bit.  Always per-pass fp32 launches on the handle's main stream, whatever bm_dbm_set_fast_binary says.
 * No parameter, particle, mean-field state or workspace of another entry point is touched.
 * Errors: Gaussian visible units, a Multinomial hidden layer, three or more hidden layers (a pass would read the OLD layer
 * above: no point of the sweep has the energy of one consistent state in the partials), a handle in literal-sigmoid mode;
 * n_temps < 1, n_chains < 1, betas not strictly increasing inside (0, 1] or betas[R-1] != 1, sweep or read before init,
 * n_steps < 1.  (No float64 counterpart.) */
int bm_dbm_pt_init(bm_dbm *h, int32_t n_chains, int32_t n_temps, const float *betas_host, const float *V0_dev, int64_t chain0);
int bm_dbm_pt_sweep(bm_dbm *h, int32_t n_steps);
int bm_dbm_pt_read(bm_dbm *h, float *V_dev, float *H1_dev, float *H2_dev, int64_t *swaps_host, int32_t *ladder_idx_host);
/* Tempered negative phase of the DBM: one update of bm_dbm_train_step whose negative particles are the beta = 1
 * rows of the chains [0, n_particles) of the ensemble bm_dbm_pt_init built, instead of the handle's persistent particles swept at
 * one temperature.  On the handle's main stream, no host synchronisation of its own (out_msre waits, as in bm_dbm_train_step):
 *   1. the v.vb and - at two hidden layers - the h2.b2 slot partials of every ensemble row are recomputed from its state and the
 *      CURRENT biases in one launch (the previous update moved the biases after the passes that left them; with unchanged
 *      biases this rewrites the same bits);
 *   2. positive phase: the mean-field loop of bm_dbm_train_step on X_dev, in the handle's arithmetic mode;
 *   3. n_gibbs_steps steps of bm_dbm_pt_sweep on ALL n_chains R rows (sites 8 + 16 t, 14 + 16 t, 9 + 16 t, 12 + 16 t of the
 *      handle's call counter; the swap parity continues the ensemble's step count);
 *   4. one gather launch copies, for every chain c < n_particles, the row at beta = 1 into particle c: v, h1 and h2 (a launch of
 *      its own because h1 is stored before the swap that settles which row is at beta = 1);
 *   5. out_msre (NULL ok): the reconstruction error of bm_dbm_train_step, before the update;
 *   6. the update of bm_dbm_train_step - gradients, sparsity, momentum, max-norm - on these statistics.
 * The call counter advances once per update, the ensemble's step count by n_gibbs_steps.  The persistent particles v, h, h_1
 * are afterwards the handed-over rows; chains beyond n_particles sweep and exchange but hand nothing over.  Every layer of the
 * ensemble is sampled, whatever sample_v_states / sample_h_states say; fast-binary mode does not apply to the tempered sweeps.
 * Errors: no ensemble, an ensemble of fewer chains than n_particles, everything bm_dbm_pt_init refuses (Gaussian visible units, a
 * Multinomial hidden layer, three or more hidden layers, literal-sigmoid mode), n_gibbs_steps < 1, a momentum buffer sharded by
 * bm_dbm_exchange_apply_direct, a handle with a communicator, a direct exchange or a mean-field all-reduce callback attached
 * (the chains are not sharded over ranks).  Float32, one process.  (No float64 counterpart.) */
int bm_dbm_train_step_pt(bm_dbm *h, const float *X_dev, float learning_rate, float momentum, int32_t n_gibbs_steps,
                         int32_t *out_n_mf, float *out_msre);
/* AIS (dbm.py:650-736; public log_Z :899-939) for a Bernoulli DBM of any
 * depth (1..4 layers): n_runs chains, n_betas temperatures, n_gibbs_steps
 * transitions per temperature.  values_host [n_runs] receives the per-chain
 * log Z estimates (host post-processing with log_mean_exp stays in Python,
 * dbm.py:935-939).  chain0 = global index of this rank's first chain (chains
 * shard over ranks).
 * Depth rule: v has depth 0, hidden layer i depth i + 1.  The chain x is the
 * odd-depth layers {h1, h3}; the even-depth layers {v, h2, h4} are summed out
 * analytically: log p*_beta(x) = beta sum_odd b.x + sum_even sum softplus(beta a),
 * log Z_0 = (V + sum n_i) log 2.  A transition updates the even-depth layers
 * given x, then the odd-depth layers given them, each in ascending depth.  For
 * two layers this is the reference's construction.
 * RNG sites (Philox, counter word site + 16 t, call = beta step, row offset =
 * global chain index): 12 for v, 8 + i for hidden layer i; x_0 ~ Ber(1/2) of
 * the j-th odd-depth layer from site 13 + 16 j, call 0.
 * The per-beta terms are fp32 as in the reference; their sum over the betas is kept in DOUBLE on the device (the
 * reference accumulates it in fp32, dbm.py:708-728, and loses nats at 1000 betas): a deliberate, documented deviation. */
int bm_dbm_ais(bm_dbm *h, int32_t n_betas, int32_t n_runs, int32_t n_gibbs_steps,
               uint64_t seed, int64_t chain0, float *values_host);
/* log_proba op (dbm.py:738-759, any depth): MF then -E_q[E] + H(mu) per row
 * of X_dev [batch_size, V] into out_host [batch_size]: sum_l sum((mu_{l-1} W_l)
 * * mu_l) (mu_{-1} = X) + X.vb + sum_l mu_l.hb_l + the entropies of every mu_l
 * (log Z is subtracted by the Python caller, dbm.py:955-956). */
int bm_dbm_log_proba(bm_dbm *h, const float *X_dev, float *out_host);

int bm_dbm_timer_start(bm_dbm *h);
int bm_dbm_timer_stop(bm_dbm *h, float *out_ms);
int bm_dbm_timer_mark(bm_dbm *h);
int bm_dbm_timer_elapsed(bm_dbm *h, float *out_ms);


/* ---- RCCL inside the library (bm_comm_init / bm_allreduce_grads; §8e: one exchange step
 * per update).  The host only transports the 128-byte id from rank 0 to the other ranks.  librccl is
 * dlopen'ed at first use (BM355_RCCL_LIB overrides the name); the single-GPU path does not need it.
 * boltzmann_machines_amd/parallel.py can drive either these or torch.distributed (bench.py default). */
typedef struct bm_comm bm_comm;
int bm_comm_unique_id(void *out_id128);                                   /* ncclGetUniqueId, rank 0 */
int bm_comm_init(int32_t rank, int32_t nranks, const void *id128, bm_comm **out);   /* on the current device */
int bm_comm_destroy(bm_comm *c);
/* in-place all-reduce(sum) / all-gather of device floats, enqueued on `stream` (a hipStream_t) */
int bm_comm_allreduce_sum(bm_comm *c, float *buf_dev, size_t count, void *stream);
int bm_comm_allgather(bm_comm *c, const float *send_dev, float *recv_dev, size_t count_per_rank, void *stream);
int bm_comm_allreduce_max(bm_comm *c, float *buf_dev, size_t count, void *stream);
int bm_comm_rank(bm_comm *c, int32_t *out_rank, int32_t *out_nranks);
/* Data-parallel DBM (dbm.py:449-452 over the GLOBAL minibatch): with a communicator installed the mean-field
 * residual of every sweep is all-reduced (max) on the device, on the handle's stream, and the device-side
 * loop control latches the same `done` on every rank - no host callback, no host synchronisation per sweep.
 * NULL removes it.  (bm_dbm_set_mf_allreduce remains for collectives the library does not own.) */
int bm_dbm_set_comm(bm_dbm *h, bm_comm *c);
/* Chain-sharded AIS (north_star): this rank runs its contiguous slice of the n_runs_total chains
 * (the chain index in the RNG stream is global), zero communication during the sweep, ONE all-gather of the
 * per-chain values at the end; values_host [n_runs_total] is filled on every rank.  Replaces the
 * session.run(log_Z) of dbm.py:930 in a multi-GPU job. */
int bm_dbm_ais_sharded(bm_dbm *h, bm_comm *c, int32_t n_betas, int32_t n_runs_total, int32_t n_gibbs_steps,
                       uint64_t seed, float *values_host);
/* the exchange step of data-parallel training: all-reduce of the handle's fused "grad" buffer on the
 * handle's stream, between bm_*_grad_step and bm_*_apply_step (no host synchronisation) */
int bm_rbm_allreduce_grads(bm_rbm *h, bm_comm *c);
/* Delayed-gradient data parallelism - a NON-parity mode (the reference is synchronous; here the update of step t is
 * the reduced gradient of step t-1), for when the all-reduce must leave the critical path.  The handle has two
 * gradient slots: bm_rbm_set_grad_slot picks the one bm_rbm_grad_step writes and bm_rbm_apply_step reads;
 * bm_rbm_allreduce_grads_async reduces the current slot on the handle's communication stream, ordered after
 * everything enqueued so far on the compute stream, and returns at once; bm_rbm_wait_grads makes the compute stream
 * wait for the reduction of a slot.  Per step t: set_grad_slot(t % 2), grad_step, allreduce_grads_async; then, for
 * t > 0: wait_grads((t-1) % 2), set_grad_slot((t-1) % 2), apply_step. */
int bm_rbm_set_grad_slot(bm_rbm *h, int32_t slot);
int bm_rbm_allreduce_grads_async(bm_rbm *h, bm_comm *c);
int bm_rbm_wait_grads(bm_rbm *h, int32_t slot);
int bm_dbm_allreduce_grads(bm_dbm *h, bm_comm *c);

/* ---- one-shot exchange over peer-mapped device memory (SURVEY §5 "Distributed communication backend": a direct
 * reduce-scatter + all-gather over the 7 xGMI links instead of a ring; §8e: the ONE exchange step of a data-parallel
 * update).  One process per GPU.  Every rank: bm_xchg_create on the buffer it wants summed -> bm_xchg_export (a
 * 256-byte blob: hipIpc handles of the buffer, a staging slice and the flag words) -> the host gathers the blobs
 * of all ranks in rank order (any channel) -> bm_xchg_attach.  bm_xchg_allreduce_sum then runs ONE kernel per rank
 * on `stream`: rank r adds slice r of every rank's buffer in rank order 0..N-1 (16-byte cache-bypassing loads over
 * all links at once), publishes it, and pulls the other slices from their owners; every rank ends with the same
 * bits.  Every wait inside the kernel is bounded (BM_XCHG_TIMEOUT_S, default 20 s); bm_xchg_status reports a
 * timed-out wait instead of a hung device.  The RCCL path (bm_comm_*) computes the same sums in ring order. */
typedef struct bm_xchg bm_xchg;
int bm_xchg_create(int32_t rank, int32_t nranks, float *buf_dev, size_t count, bm_xchg **out);
int bm_xchg_blob_bytes(void);                                            /* 256 */
int bm_xchg_export(bm_xchg *x, void *out_blob256);
int bm_xchg_attach(bm_xchg *x, const void *all_blobs /* nranks x 256 bytes, ordered by rank */);
int bm_xchg_destroy(bm_xchg *x);
int bm_xchg_allreduce_sum(bm_xchg *x, void *stream);
/* all-reduce(max) of ONE non-negative float in this rank's device memory: one 8-byte {value, epoch} store into
 * every peer's slot, one fabric hop (the mean-field residual of a data-parallel DBM, dbm.py:449-452) */
int bm_xchg_allreduce_max1(bm_xchg *x, float *val_dev, void *stream);
int bm_xchg_status(bm_xchg *x, int32_t *out_status);                     /* synchronises; 0 = no wait timed out */
int bm_xchg_set_timeout(bm_xchg *x, double seconds);                     /* bound of the in-kernel waits of later launches */
/* at most n workgroups per exchange launch (default: up to one per CU); before the first exchange.  Only for ranks that
 * SHARE a device (dry runs): workgroups spinning on every CU can keep the peer process's kernels from being placed. */
int bm_xchg_set_max_workgroups(bm_xchg *x, int32_t n);
int bm_xchg_info(bm_xchg *x, int32_t *out_rank, int32_t *out_nranks, size_t *out_count);
/* the handle's fused "grad" buffer as the exchanged buffer; bm_*_allreduce_grads_direct is the drop-in for
 * bm_*_allreduce_grads between bm_*_grad_step and bm_*_apply_step */
int bm_rbm_xchg_create(bm_rbm *h, int32_t rank, int32_t nranks, bm_xchg **out);
int bm_dbm_xchg_create(bm_dbm *h, int32_t rank, int32_t nranks, bm_xchg **out);
int bm_rbm_allreduce_grads_direct(bm_rbm *h, bm_xchg *x);
int bm_dbm_allreduce_grads_direct(bm_dbm *h, bm_xchg *x);
/* Data-parallel CD-k, the exchange AND the parameter update in ONE launch (replaces bm_rbm_allreduce_grads_direct +
 * bm_rbm_apply_step; same bits): rank r sums slice r of the W part of every rank's gradient buffer in rank order,
 * applies g = raw / N - l2 W - pen, dW = lr (mom dW + g), W += dW (base_rbm.py:446-468) to ITS slice of W / dW and
 * every rank gathers the updated slices of W; the [V | H | H] tail is reduced by every rank itself (rank order) and
 * the bias / q_means update applied to every replica.  After it all replicas hold the same W, vb, hb, dvb, dhb,
 * q_means; of the momentum buffer dW a rank holds its own slice - bm_rbm_exchange_gather_dw completes the replicas
 * (call it before dW is read: checkpoints, get_param("dW")).  Needs n_hidden % 4 == 0. */
int bm_rbm_exchange_apply_direct(bm_rbm *h, bm_xchg *x, int32_t B_global, float learning_rate, float momentum);
int bm_rbm_exchange_gather_dw(bm_rbm *h, bm_xchg *x);
/* The same for the data-parallel DBM update (replaces bm_dbm_allreduce_grads_direct + bm_dbm_apply_step; same bits), with
 * COLUMN-sliced ownership because the update ends with the max-norm rescale of whole columns (dbm.py:511-513, 603-606):
 * rank r owns columns [r sw_i, (r + 1) sw_i) of every W_i (sw_i = 32 ceil(n_{i+1} / (32 nranks))).  One launch sums the
 * owned columns of the raw outer products over the ranks (rank order), applies the update to them and - every rank for
 * itself - the bias / q_means / mu_means / penalty update from the reduced column sums (dbm.py:550-600); the max-norm
 * kernels run on the owned columns; a second launch gathers the other ranks' columns into W_i, W_i^T and the column norms.
 * The momentum buffers dW_i stay with their owners: bm_dbm_get_param("dW"), bm_dbm_train_step and bm_dbm_apply_step fail
 * until bm_dbm_exchange_gather_dw.  Needs every hidden width to be a multiple of 4 and the exchange created by
 * bm_dbm_xchg_create for this engine (its staging slice is sized for the columns): bm_dbm_exchange_apply_ok says. */
int bm_dbm_exchange_apply_ok(bm_dbm *h, bm_xchg *x, int32_t *out_ok);
int bm_dbm_exchange_apply_direct(bm_dbm *h, bm_xchg *x, int32_t N_global, int32_t M_global, float learning_rate, float momentum);
int bm_dbm_exchange_gather_dw(bm_dbm *h, bm_xchg *x);
/* bm_dbm_ais_sharded over the direct exchange instead of the RCCL communicator (same slices, same values bit for bit): the
 * per-chain values travel through the exchange's registered buffer as an all-reduce(sum) of a window in which every rank
 * wrote its own chains and zeros elsewhere (x + 0 = x: every rank receives the owner's bits).  Overwrites the head of the
 * engine's gradient payload (recomputed by every update).  A rank whose sweep fails contributes NaN and every rank
 * reports the error; a rank that never arrives ends the wait at the exchange's time-out (sticky status). */
int bm_dbm_ais_sharded_direct(bm_dbm *h, bm_xchg *x, int32_t n_betas, int32_t n_runs_total, int32_t n_gibbs_steps,
                              uint64_t seed, float *values_host);
/* Opt-in "fast-binary" mode (SURVEY §7 hard part 4; csrc/bm_bf3.h): contractions whose input states are {0,1}
 * bitmaps (AIS with all layers sampled; the RBM sampling sweep with both layers sampled; in the PCD particle sweeps of
 * bm_dbm_train_step / bm_dbm_sample_v every contraction over a Bernoulli layer sampled earlier in the same call - a
 * real-valued visible layer and the particles a call starts from are read in fp32) split the fp32 weights
 * EXACTLY into three bf16 planes and run on the bf16 matrix cores - exact products, fp32 accumulation in a
 * different order than the default chain: results agree to fp32 round-off (free energy / log-weights 1e-5, bitmaps
 * identical except where |u - p| is at round-off distance), NOT bit for bit.  Never the default.
 * AIS in this mode: 2-layer DBMs only; at other depths bm_dbm_ais runs the fp32 path (the default's values, bit for bit).
 * on = 1: where the mode was measured FASTER than the fp32 path - AIS always; the sampling sweep of an RBM and the particle
 * sweeps of a DBM only from 8M weights in the (bottom) weight matrix upwards (3072 x 5000 gains, 784 x 1024 loses: there the
 * passes are bound by their fill and epilogue, not by matrix time).  on = 2: wherever legal (tests, measurements). */
int bm_dbm_set_fast_binary(bm_dbm *h, int32_t on);
int bm_rbm_set_fast_binary(bm_rbm *h, int32_t on);
/* bm_dbm_ais accumulation.  0 (default): per chain the DIFFERENCE log p*_b(x) - log p*_a(x) of consecutive betas, its
 * row sums and the running log-weight in double, in a fixed order.  1: LITERALLY the reference's float32 arithmetic
 * (dbm.py:650-660, :708-728): each log p*_beta(x) formed in float32 and added to / subtracted from a float32
 * log-weight in the graph's order; two extra score-only passes per beta. */
int bm_dbm_set_ais_literal(bm_dbm *h, int32_t on);
/* Sigmoid of the Bernoulli layers.  0 (default): the engine's form (one correctly rounded division, e / (1 + e) for x < 0;
 * ~1.4 ulp).  1: LITERALLY tf.nn.sigmoid as the reference evaluates it (layers.py:47-48 -> float32 1 / (1 + exp(-x)), exp
 * as Eigen's pexp of TensorFlow 1.3; ~1.8 ulp) in every pass of this engine: the same values to float32 round-off, and the
 * reference's mean-field trip counts - the loop of dbm.py:449-452 at mf_tol = 1e-7 is decided in the last bits of the
 * means (784-512-1024: 5 - 6 sweeps per update with the literal form, 7 - 8 with the default). */
int bm_dbm_set_sigmoid_literal(bm_dbm *h, int32_t on);
/* ---- Centred training (Montavon & Mueller 2012; Melchior, Fischer & Wiskott 2016) -------------------
 * The model stays in standard parameters (W, vb, hb); only the update changes.  With layers x_0 = v, x_1 .. x_L, offsets o_l
 * (one vector per layer) and sliding factors nu_l, one update runs, in this order:
 *   o_l  <- (1 - nu_l) o_l + nu_l colmean_pos(x_l)
 *   g_l   = colsum_pos(x_l) / N - colsum_neg(x_l) / M                        (the plain bias gradient)
 *   dW_l  = pos / N - neg / M - o_{l-1} g_l^T - g_{l-1} o_l^T                 (then l2, sparsity, momentum, lr, max-norm as ever)
 *   a_lb  = (x_lb - o_l) . o_l                                               (one scalar per row and layer, both phases)
 *   r_l   = (1/N) sum_pos (x_lb - o_l)(a_{l-1,b} + a_{l+1,b}) - (1/M) sum_neg (same);   bias gradient g_l - r_l
 * which is the gradient of the centred parameterisation expressed in the standard one.  The mode is a property of the
 * handle: while it is on, every fused update entry takes the centred update - bm_rbm_train_step, _metrics, _metrics_async,
 * bm_rbm_train_epoch, bm_rbm_train_step_pt, bm_rbm_train_epoch_pt; bm_dbm_train_step, bm_dbm_train_step_pt.  Sampling,
 * mean-field, AIS, tempering and the metrics are untouched.  With all offsets and sliding factors zero the update is the plain
 * one, bit for bit.  The offsets are variables of bm_*_set_param / get_param: "ov", "oh" (RBM); "ov", "oh", "oh_1", ...
 * (DBM); they are zero until set.  Sliding factors lie in [0, 1].
 * Refused (the error names centering): switching it on for Gaussian visible units, Multinomial hidden units, dbm_first /
 * dbm_last handles or handles with dropout; and, while it is on, the split and exchange paths - bm_*_grad_step,
 * bm_*_apply_step, bm_*_exchange_apply_direct.  The float64 engines have no centred update. */
int bm_rbm_set_centering(bm_rbm *h, int32_t on, float nu_v, float nu_h);
int bm_dbm_set_centering(bm_dbm *h, int32_t on, const float *nu /* [n_layers + 1]: v, h_1, ...; read when on != 0 */);
/* ---- Class head of a Bernoulli RBM (Larochelle & Bengio 2008, classification RBMs) ---------------------
 * A head of C classes on the RBM's hidden layer: U [C][H] and yb [C] beside the RBM's own W, hb, vb, with
 *   z_i = (x W)_i + hb_i,   s_c = yb_c + sum_i softplus(z_i + U[c][i]),   log p(c|x) = s_c - logsumexp_c' s_c'
 * - the exact class posterior of the RBM over (x, one-hot y) - and the exact gradient of the batch mean of log p(t|x), which
 * the train entries ascend (no sampling, no RNG: the call counter of the handle's streams is not touched):
 *   coef[j][c] = 1[c == t_j] - p(c|x_j),   S[j][c][i] = sigmoid(z_ji + U[c][i]),   g = S[., t, .] - sum_c p(c|x) S[., c, .]
 *   dW = X^T g / B,  dhb = colmean(g),  dvb = 0,  dU[c][i] = sum_j coef[j][c] S[j][c][i] / B,  dyb[c] = colmean(coef[:, c])
 * with the update rules of bm_rbm_train_step: W and U take l2, momentum and the learning rate as W does there, hb and yb the
 * bias rule; vb sees a zero gradient (its momentum buffer decays under the ordinary rule).  q_means follows the rule of
 * bm_rbm_train_step on the model's class-averaged hidden means.
 * bm_rbm_set_classes: C >= 2 attaches a head - U, yb and the momentum buffers dU, dyb, all zero, and workspaces for max_batch
 * rows; an attached head is replaced.  C == 0 detaches it.  While a head is attached "U", "dU" ([C][H], dense, row-major), "yb",
 * "dyb" are variables of bm_rbm_set_param / get_param / dev_ptr.  Everything else the handle does is unchanged by a head.
 * bm_rbm_class_log_proba: log p(c|x) [B][C] of B rows (any B: the workspaces grow on demand) to the host; synchronises.
 * bm_rbm_class_train_step: one update from X_dev [B][V] and the labels y_dev (int32 [B], device), B <= max_batch.  out2
 * (nullable): the batch mean of log p(t|x) and the accuracy, both of the forward pass BEFORE the update; with out2 the call
 * synchronises, without it it only queues.  bm_rbm_class_train_epoch: N rows as consecutive batches of `batch` rows, the same
 * launches as the caller's own loop over the step entry, no host wait between batches; out2 averaged over the N rows.
 * Every sum runs in a fixed order: the results do not depend on the run or on the tile geometry.
 * A label outside [0, C) never indexes memory: its row contributes nothing to the update (the divisor stays B), and the
 * next bm_rbm_sync, or the out2 fetch, returns an error once and clears the flag.
 * Refused with an error: no head attached; Gaussian visible or Multinomial hidden units; dbm_first / dbm_last handles; and for
 * the train entries dropout, sparsity_cost != 0, centering switched on, a handle that takes part in a data-parallel run,
 * B > max_batch.  The float64 engines have no class head. */
int bm_rbm_set_classes(bm_rbm *h, int32_t n_classes);
int bm_rbm_class_log_proba(bm_rbm *h, const float *X_dev, int32_t B, float *logp_host /* [B][n_classes] */);
int bm_rbm_class_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [B] */, int32_t B, float learning_rate,
                            float momentum, float *out2 /* nullable */);
int bm_rbm_class_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [N] */, int64_t N, int32_t batch,
                             float learning_rate, float momentum, float *out2 /* nullable */);
/* ---- Fine-tuning a stack of layers below the head by back-propagation -------
 * D >= 0 feature layers under a classification RBM, every layer a bm_rbm handle of its own (Bernoulli-Bernoulli, float32):
 *   a_0 = x,   a_l = sigmoid(a_{l-1} W_l + hb_l)  (l = 1..D; means only, nothing is sampled)
 *   log p(c|x) = the exact posterior above of the top handle on the input a_D
 * The train entries ascend the batch mean of log p(t|x).  With g = pos + negm of the top handle and ' marking pre-update values:
 *   delta_D = (g W_top'^T) .* a_D .* (1 - a_D),      delta_l = (delta_{l+1} W_{l+1}'^T) .* a_l .* (1 - a_l)
 *   layer l:  dW_l = a_{l-1}^T delta_l / B,  dhb_l = colmean(delta_l),  dvb_l = 0;   top: bm_rbm_class_train_step on the input a_D
 * W, W^T, hb and their momentum buffers of a layer go through that handle's own fused update (its l2, its rules); its vb sees a
 * zero gradient.  Every backward pass reads pre-update weights.  The handles keep their streams; the launches are ordered across
 * them with events, so the caller needs no synchronisation between the handles.
 * bm_rbm_backprop_down: Out [B][V] (pitch ldo) = (Delta [B][H] W^T) .* A .* (1 - A) of handle h, A [B][V] (pitch lda) an activation
 *   matrix; A_dev == NULL stores Delta W^T itself.  Each product and the difference are rounded once: (z * a) * (1 - a).  Any
 *   B <= max_batch.  Queues only.
 * bm_rbm_delta_update: W, W^T, hb of handle h from its input X [B][V] and a delta [B][H] (both dense): dW = X^T Delta / B,
 *   dhb = colmean(Delta), dvb = 0, through the fused update of bm_rbm_train_step.  Queues only.
 * bm_rbm_class_stack_train_step: one update of the whole stack.  `below`: the n_below handles under the top, bottom first;
 *   learning_rate [n_below + 1]: one value per layer, the top's last.  out2 as in bm_rbm_class_train_step: with it the call waits
 *   for every layer's stream, without it it only queues (then synchronise EVERY handle before reading its variables).  n_below == 0
 *   issues exactly the launches of bm_rbm_class_train_step.  bm_rbm_class_stack_train_epoch: N rows as consecutive batches of
 *   `batch` rows, the same launches as the caller's loop over the step entry, no host wait between the batches.
 * bm_rbm_class_stack_log_proba: log p(c|x) [B][C] of B rows (any B: rows go up the stack in slices no longer than the smallest
 *   max_batch below the top) to the host; synchronises.
 * A label outside [0, C) behaves as above: its row has zero g, hence a zero delta in every layer, and the flag is raised.
 * Refused with an error, for every handle of the stack: what bm_rbm_class_train_step refuses (Gaussian, Multinomial, dbm_first /
 * dbm_last, dropout, sparsity_cost != 0, centering, a data-parallel handle, B > max_batch); widths that do not chain
 * (H of a layer != V of the one above); the same handle twice; no head on the top. */
int bm_rbm_backprop_down(bm_rbm *h, const float *Delta_dev, int32_t B, const float *A_dev /* nullable */, int32_t lda, float *Out_dev,
                         int32_t ldo);
int bm_rbm_delta_update(bm_rbm *h, const float *X_dev, const float *Delta_dev, int32_t B, float learning_rate, float momentum);
int bm_rbm_class_stack_train_step(bm_rbm *top, bm_rbm *const *below /* [n_below], bottom first */, int32_t n_below, const float *X_dev,
                                  const int32_t *y_dev /* [B] */, int32_t B, const float *learning_rate /* [n_below + 1] */,
                                  float momentum, float *out2 /* nullable */);
int bm_rbm_class_stack_train_epoch(bm_rbm *top, bm_rbm *const *below, int32_t n_below, const float *X_dev, const int32_t *y_dev /* [N] */,
                                   int64_t N, int32_t batch, const float *learning_rate /* [n_below + 1] */, float momentum,
                                   float *out2 /* nullable */);
int bm_rbm_class_stack_log_proba(bm_rbm *top, bm_rbm *const *below, int32_t n_below, const float *X_dev, int32_t B,
                                 float *logp_host /* [B][n_classes] */);
/* a_D of B rows (any B, in the same slices) into the DEVICE matrix A_dev [B][H_D] (dense); n_below >= 1; synchronises */
int bm_rbm_stack_transform(bm_rbm *const *below, int32_t n_below, const float *X_dev, int32_t B, float *A_dev);
/* ---- joint training of the classification RBM and sampling by class --------
 * The RBM over (x, one-hot y) with the head's own parameters, nothing new is stored:
 *   p(h_i = 1 | x, y) = sigmoid((x W)_i + hb_i + U[y][i]),   p(x | h) = the RBM's visible pass,
 *   p(y = c | h) = softmax_c(yb_c + sum_i h_i U[c][i])
 * bm_rbm_class_joint_train_step: one update of L_gen + disc_weight * L_disc from X_dev [B][V] and y_dev (int32 [B], device).
 * L_gen is the CD-k estimate of the gradient of log p(x, y): h0 from (x, y), per Gibbs step the visible pass and a class draw
 * from the same hidden input, then the prop-up given (v_k, y_k); W, hb, vb take the update of bm_rbm_train_step on
 * (X, h0) and (v_k, h_k), U and yb the rules of bm_rbm_class_train_step on
 *   dU[c][i] = (1/B) sum_j (1[y_j = c] h0_ji - 1[yk_j = c] hk_ji + disc_weight coef_jc sigmoid(t_ji + U[c][i])),
 *   dyb[c]   = (1/B) sum_j (1[y_j = c] - 1[yk_j = c] + disc_weight coef_jc).
 * L_disc is the objective of bm_rbm_class_train_step (Larochelle & Bengio's hybrid objective L_disc + alpha L_gen with
 * disc_weight = 1 / alpha folded into the learning rate); with disc_weight == 0 none of its launches run unless out2 is asked
 * for.  One application of the update rules per batch; the call counter of the handle's streams advances by one per update,
 * as in bm_rbm_train_step.  out2 as in bm_rbm_class_train_step.  bm_rbm_class_joint_train_epoch: N rows as consecutive
 * batches, no host wait between them.  Every sum runs in a fixed order: two runs give identical bits.
 * bm_rbm_class_joint_chain: the chain of one such update without the update (one call of the streams), its states to the
 * host, dense - E[h | x, y] and its draw, v_k, y_k, E[h | v_k, y_k]; any pointer may be null; synchronises.
 * bm_rbm_class_gibbs: class-conditional sampling.  n_steps of h ~ p(h | v, y), v ~ p(v | h) with y (int32 [B], device)
 * clamped, from V_dev (dense [B][V]) or - null - from v_0 ~ Ber(1/2); the last states to out_v, the last visible means to
 * out_vmeans (nullable), both dense device buffers.  Both layers are always sampled; rows draw by global position
 * (bm_rbm_set_row_offset): the result does not depend on how the rows are sliced.  One call of the streams.
 * A label outside [0, C) never indexes memory: its row takes the plain hidden bias, is out of the U / yb sums, and the next
 * bm_rbm_sync or out2 fetch returns an error once.
 * Refused with an error: what bm_rbm_class_train_step refuses; n_gibbs_steps < 1; disc_weight < 0. */
int bm_rbm_class_joint_train_step(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [B] */, int32_t B, int32_t n_gibbs_steps,
                                  float learning_rate, float momentum, float disc_weight, float *out2 /* nullable */);
int bm_rbm_class_joint_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [N] */, int64_t N, int32_t batch,
                                   int32_t n_gibbs_steps, float learning_rate, float momentum, float disc_weight,
                                   float *out2 /* nullable */);
int bm_rbm_class_joint_chain(bm_rbm *h, const float *X_dev, const int32_t *y_dev, int32_t B, int32_t n_gibbs_steps,
                             float *h0_means_host, float *h0_states_host, float *vk_host, int32_t *yk_host, float *hk_means_host);
int bm_rbm_class_gibbs(bm_rbm *h, const float *V_dev /* nullable */, const int32_t *y_dev /* [B] */, int32_t B, int32_t n_steps,
                       float *out_v, float *out_vmeans /* nullable */);
/* ---- semi-supervised training of the classification RBM --------------------
 * bm_rbm_class_unsup_train_step: one update on B UNLABELLED rows X_dev [B][V]: ascent of the batch mean of
 * log p(x) = log sum_y p(x, y) of the joint model.  The positive phase over y is exact - with p_jc = p(c | x_j) of
 * bm_rbm_class_log_proba, t = x W + hb and S_jci = sigmoid(t_ji + U[c][i]): em_ji = sum_c p_jc S_jci = E[h_i | x_j] - the
 * negative phase is the CD-k chain of bm_rbm_class_joint_train_step started at y0_j ~ p(y | x_j):
 *   dW = (X^T em - v_k^T h_k) / B,  dhb = colmean(em - h_k),  dvb = colmean(X - v_k),
 *   dU[c][i] = (1/B) sum_j (p_jc S_jci - 1[yk_j = c] hk_ji),   dyb[c] = (1/B) sum_j (p_jc - 1[yk_j = c]),
 * all from the OLD parameters, through the update rules of bm_rbm_class_joint_train_step.  The call counter advances by one.
 * out2 (nullable): the mean posterior entropy -sum_c p_jc log p_jc and the mean max_c p_jc of the forward pass before the
 * update.  Every sum runs in a fixed order: two runs give identical bits.
 * bm_rbm_class_unsup_chain: the chain and the positive operand of one such update without the update (one call of the
 * streams), to the host, dense - y0, em, the draw of h0 ~ p(h | x, y0), v_k, y_k, E[h | v_k, y_k]; any pointer may be null;
 * synchronises.
 * bm_rbm_class_semi_train_epoch: N labelled rows as consecutive batches, no host wait between them; behind every labelled
 * batch's joint update (learning_rate, disc_weight) one unlabelled update with learning_rate * unl_weight (one float product)
 * on the next slice of Xu_dev [Nu][V]: its consecutive slices of `batch` rows (a short last one) are taken cyclically,
 * starting at slice u_slice.  This is stochastic gradient ascent on L_sup + unl_weight * L_unsup with alternating minibatches
 * (DESIGN.md 3.20 says why it is not one combined update).  out4 (nullable): out2 of bm_rbm_class_joint_train_epoch, then the
 * unlabelled pair, each a mean over its own rows.  unl_weight == 0: no unlabelled launch, Xu_dev may be null, the result is
 * bm_rbm_class_joint_train_epoch's bit for bit.
 * Refused with an error: what bm_rbm_class_joint_train_step refuses; unl_weight < 0; Nu < 1 or a null Xu_dev while
 * unl_weight > 0; u_slice outside [0, ceil(Nu / batch)). */
int bm_rbm_class_unsup_train_step(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps, float learning_rate, float momentum,
                                  float *out2 /* nullable */);
int bm_rbm_class_unsup_chain(bm_rbm *h, const float *X_dev, int32_t B, int32_t n_gibbs_steps, int32_t *y0_host, float *em_host,
                             float *h0_states_host, float *vk_host, int32_t *yk_host, float *hk_means_host);
int bm_rbm_class_semi_train_epoch(bm_rbm *h, const float *X_dev, const int32_t *y_dev /* [N] */, int64_t N,
                                  const float *Xu_dev /* [Nu][V], nullable */, int64_t Nu, int64_t u_slice, int32_t batch,
                                  int32_t n_gibbs_steps, float learning_rate, float momentum, float disc_weight, float unl_weight,
                                  float *out4 /* nullable */);
/* ---- float64 DBM path ----------------------------------------------------------------------
 * DBM(dtype='float64') (base/mixin.py:14-25; the DBM graph is built "all in model dtype", dbm.py:294-383): the fetch sites
 * of the float32 entry points above with every buffer, hyper-parameter and random draw in double, on the FP64 tile engine of
 * the float64 RBM path (sequential ascending-k fma chains: bit-identical to oracle/bm_oracle_dbm64.c for everything that
 * feeds back into state).  A compatibility path (csrc/bm_dbm64.hip): Bernoulli hidden layers, Bernoulli or Gaussian visible
 * units, one process; the mean-field loop is driven by the host.  Variables as in bm_dbm_set_param.
 * hyper12 = {mf_tol, l2, max_norm, sparsity_damping, sparsity_target[4], sparsity_cost[4]} as doubles (NULL: from cfg). */
typedef struct bm_dbm64 bm_dbm64;
int bm_dbm64_create(const bm_dbm_config *cfg, const double *hyper12, bm_dbm64 **out);
int bm_dbm64_destroy(bm_dbm64 *h);
int bm_dbm64_sync(bm_dbm64 *h);
int bm_dbm64_seed(bm_dbm64 *h, uint64_t seed);                                           /* tf_model.py:20-21 */
int bm_dbm64_set_row_offset(bm_dbm64 *h, int64_t row0, int64_t particle0);
int bm_dbm64_set_param(bm_dbm64 *h, const char *name, const double *host, size_t n);     /* tf_model.py:22-28 */
int bm_dbm64_get_param(bm_dbm64 *h, const char *name, double *host, size_t n);           /* tf_model.py:183-202 */
int bm_dbm64_train_step(bm_dbm64 *h, const double *X_dev, double learning_rate, double momentum,   /* dbm.py:805 */
                        int32_t n_gibbs_steps, int32_t *out_n_mf, double *out_msre);
int bm_dbm64_metrics(bm_dbm64 *h, const double *X_dev, int32_t n_gibbs_steps, int32_t *out_n_mf, double *out_msre);   /* dbm.py:813 */
int bm_dbm64_mean_field(bm_dbm64 *h, const double *X_dev, double *out_dev, int32_t *out_n_mf);   /* dbm.py:866 */
int bm_dbm64_reconstruct(bm_dbm64 *h, const double *X_dev, double *R_dev);                        /* dbm.py:881 */
int bm_dbm64_sample_v(bm_dbm64 *h, int32_t n_gibbs_steps, double *V_dev);                         /* dbm.py:892 */
int bm_dbm64_ais(bm_dbm64 *h, int32_t n_betas, int32_t n_runs, int32_t n_gibbs_steps, uint64_t seed, int64_t chain0,
                 double *values_host);                                                            /* dbm.py:930 */
int bm_dbm64_log_proba(bm_dbm64 *h, const double *X_dev, double *out_host);                       /* dbm.py:953 */

/* like bm_dbm_set_comm, with the per-sweep residual max going through bm_xchg_allreduce_max1; NULL removes it */
int bm_dbm_set_xchg(bm_dbm *h, bm_xchg *x);

#ifdef __cplusplus
}
#endif
#endif /* BM355_H */
