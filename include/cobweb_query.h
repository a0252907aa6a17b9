/*
 * cobweb_query.h -- C ABI of libcwq, the MI355X (gfx950) query engine for the
 * Cobweb retrieval path of Teachable-AI-Lab/RAG-Cobweb (reference @ 2025-09-26).
 *
 * The reference exposes no native boundary: its interface is the Python class
 * CobwebWrapper (src/cobweb/CobwebWrapper.py).  Each entry point below replaces
 * one op sequence of that class (file:line cited per function).  The Python
 * drop-in (rag-cobweb_amd/wrapper.py) binds these symbols with ctypes.
 *
 * Conventions
 *   - Every function returns int status: CWQ_OK (0) or a negative CWQ_ERR_*;
 *     cwq_last_error() returns a thread-local message for the last failure.
 *   - Pointers documented "device" are HIP device pointers (e.g. a torch tensor's
 *     data_ptr()); "host" pointers are ordinary CPU memory.  Outputs are written
 *     into caller-allocated buffers; the library never frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     query calls are stream-ordered and asynchronous unless stated otherwise.
 *   - Node numbering is the reference's BFS order (CobwebWrapper.py:107-132):
 *     node 0 is the root and the children of a node are consecutive, in the
 *     order of its children list.  Sentence ids are the reference's sentence ids.
 *   - A handle serialises its query calls (host mutex) and owns one device
 *     workspace.  Calls may be issued on different streams: each call makes its
 *     stream wait for the previous call's work (an event recorded at the end of every
 *     call), so the workspace is never shared by two in-flight calls.  For concurrent
 *     execution use one handle per stream.
 */
#ifndef COBWEB_QUERY_H
#define COBWEB_QUERY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWQ_OK 0
#define CWQ_ERR_ARG (-1)        /* invalid argument / malformed tree            */
#define CWQ_ERR_HIP (-2)        /* HIP runtime error                            */
#define CWQ_ERR_OOM (-3)        /* device allocation failed                     */
#define CWQ_ERR_NOT_FOUND (-4)  /* categorize retrieved < k nodes (the reference
                                   raises IndexError, CobwebTorchTree.py:289)    */

typedef struct cwq_index cwq_index;

/* Library version (major*10000 + minor*100 + patch). */
int cwq_version(void);

/* Build id: a hash of the sources, this header and the compile flags the library was
 * built from (rag-cobweb_amd/build.py); the Python binding refuses a library whose id
 * differs from the sources next to it. */
const char* cwq_build_id(void);

/* Thread-local message describing the last error on this thread. */
const char* cwq_last_error(void);

/*
 * Build the immutable query index from a flattened tree.
 * Replaces CobwebWrapper.build_prediction_index (CobwebWrapper.py:91-208): the
 * caller passes the BFS-ordered node statistics the reference caches in
 * _node_means / _node_vars (:186-203) and the structure the reference keeps in
 * _index_to_node / _leaf_to_path_indices / _path_matrix (:107-184).
 *
 *   device            HIP device ordinal the index lives on
 *   n_nodes, dim      Nn nodes of dimension D
 *   mean, var         device, [n_nodes*dim] fp32 row-major; var = compute_var
 *                     (meanSq/count + prior_var, or prior_var for empty nodes)
 *   parent            host, [n_nodes] int64; parent[0] = -1 and parent is
 *                     non-decreasing (BFS order)
 *   node_of_sentence  host, [n_sent] int64; the BFS node holding sentence id s
 *                     (-1: the sentence is not in the tree)
 *   level_w, n_w      host level weights (CobwebWrapper.py:153-166); depth >= n_w
 *                     uses 1.0; each path term is weighted level_w[depth]/len(path)
 *   stream            stream for the build kernels (the call synchronises it)
 */
int cwq_index_create(int device, int64_t n_nodes, int32_t dim, const float* mean, const float* var,
                     const int64_t* parent, const int64_t* node_of_sentence, int64_t n_sent,
                     const double* level_w, int32_t n_w, void* stream, cwq_index** out);

/*
 * cwq_index_create with the variances in compact form (same index, same results).
 * In the reference every count-1 leaf has var = meanSq/1 + prior_var = prior_var in all
 * D dimensions (CobwebTorchTree.py:336-342, CobwebWrapper.py:186-203), so a flat 10M x
 * 1024 tree's _node_vars is 41 GB of one repeated value.  Here:
 *   var_row   device [n_nodes] fp32: the variance of node i in every dimension, for the
 *             nodes NOT listed in an_nodes
 *   an_nodes  host [n_an] int64: the nodes whose variances differ across dimensions
 *             (internal nodes, leaves holding several points), each listed once
 *   an_var    device [n_an*dim] fp32: their compute_var rows, in an_nodes order
 * Other arguments as cwq_index_create.  The caller may free every input on return.
 */
int cwq_index_create_cv(int device, int64_t n_nodes, int32_t dim, const float* mean, const float* var_row,
                        const int64_t* an_nodes, int64_t n_an, const float* an_var, const int64_t* parent,
                        const int64_t* node_of_sentence, int64_t n_sent, const double* level_w, int32_t n_w,
                        void* stream, cwq_index** out);

int cwq_index_destroy(cwq_index* idx);

/* Index facts: out[0]=n_nodes out[1]=dim out[2]=n_sent out[3]=internal nodes
 * out[4]=leaf-class rows out[5]=isotropic rows out[6]=max depth out[7]=device bytes
 * (the handle's own copies; the workspace grows on demand up to 40% of the free device
 * memory, 2-48 GiB, per call; CWQ_WS_BUDGET_MB overrides).
 * Device footprint per node row: internal nodes 8*DP B (1/sigma, mu/sigma), isotropic
 * leaf rows 4*DP (dim-major mean) + 4*DP (row-major mean) + 2*DPB (bf16) + 32 B,
 * anisotropic leaf rows 8*DP B; C3 (1M x 768) 7.8 GB, C4 (10M x 1024) 104 GB -- the
 * largest flat tree one 288 GB MI355X holds is ~25M x 1024 (the caller may free its
 * mean/var tensors after cwq_index_create). */
int cwq_index_info(const cwq_index* idx, int64_t* out8);

/* How the filters centre their rows (no reference counterpart: a property of this
 * index's bf16 filter operands): out[0] = 1 when isotropic rows are stored centred at
 * their group centre's mean (clustered trees, cwq_group.hip; CWQ_GROUP_CENTRE=0 / 1 at
 * index creation: off / on wherever it applies), out[1] = groups, out[2] = group-centred
 * rows, out[3] = 1 when the per-call int8 panel was built, out[4] = the hub rows of the
 * batch filter's threshold sample (the rows with the largest query-independent key term,
 * appended to the strided sample; CWQ_FG_HUB_DIV = n at index creation: NL_iso / n rows,
 * 0: none), out[5] = the batch filter's launch schedule on this index by the default rules
 * (0: bf16 launches only, 1: int8 from a quarter of the row tiles on, 2: the early schedule,
 * bf16 sample pass and every launch on the int8 operands, 3: the direct schedule, int8
 * sample pass with exact-key thresholds, every launch on the int8 operands), out[6] = 1 when the last
 * Fast batch call ran the direct schedule. */
int cwq_index_filter_info(const cwq_index* idx, int64_t* out7);

/* The tree-adaptive cut the index chose (no reference counterpart): out[0] =
 * groups (centre nodes; 0: none planned), out[1] = top nodes (the root and the centres'
 * ancestors, computed exactly by every pruned query), out[2] = the deepest centre's depth,
 * out[3] = groups whose rows qualify for centring at their centre.  CWQ_GROUP_CUT=1 at index
 * creation keeps the depth-1 cut. */
int cwq_index_cut_info(const cwq_index* idx, int64_t* out4);

/* After cwq_categorize / cwq_categorize_host (no reference counterpart): out[0] =
 * queries replayed straight away by the exact lazy replay (a call of <= 64 queries on an
 * index whose list paths left every query of the last calls to the DENSE re-run; env
 * CWQ_CAT_DIRECT=0 / 1: never / always), out[1] = queries whose DENSE re-run was that lazy
 * replay (leaf rows scored when their parent is popped; CWQ_CAT_LAZY=0: the materialised
 * form).  Either way the pop order, n_found and call counts are the heap search's. */
int cwq_last_lazy_stats(const cwq_index* idx, int64_t* out2);

/*
 * "Cobweb Fast" batched top-k (A6).  Replaces CobwebWrapper.cobweb_predict_indexed
 * (CobwebWrapper.py:210-265, alias cobweb_predict_fast :428-433) for nq queries:
 * score(s) = sum over the root->leaf path of (w[depth]/len) * lp'(node), with
 * lp'(n) = -0.5*(sum_d log v + sum_d (x-mu)^2/v) (:230-241); top-k descending.
 *   q        device [nq*dim] fp32 queries
 *   ids      device [nq*k] int64 sentence ids (-1 past the number of sentences)
 *   scores   device [nq*k] fp32 scores (may be NULL)
 * Ties are broken by lower node index, then lower sentence id (the reference
 * adds randn*1e-6 noise instead, :246-256).  Any k >= 1 is accepted; k >= n_sent
 * returns the full ranking like the reference's argsort branch (:246-251).
 */
int cwq_score_topk(cwq_index* idx, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                   void* stream);

/*
 * All sentence scores (A8).  Replaces CobwebWrapper.cobweb_rank_scores
 * (CobwebWrapper.py:267-294).  out: device [nq*n_sent] fp32 (sentences that are
 * not in the tree get -inf).
 */
int cwq_rank_scores(cwq_index* idx, const float* q, int64_t nq, float* out, void* stream);

/*
 * Backward of cwq_rank_scores: the reference documents cobweb_rank_scores as
 * "Differentiable: return raw scores for all leaves" (CobwebWrapper.py:267-294), and its
 * query-encoder training backpropagates a cross-entropy loss through the scores into the
 * query embedding (src/training/cobweb_query_train.py:104-126).
 *   grad_out: device [nq*n_sent] fp32, the upstream gradient of every score.  Entries of
 *             sentences that are not in the tree (score -inf) are never read.
 *   grad_q:   device [nq*dim] fp32, d(sum grad_out * scores)/dq.
 * Needs no state of the forward call.  fp32 means throughout; no float atomics: the result
 * is identical from run to run and a query's gradient does not depend on the batch it is
 * in.  CWQ_ERR_ARG on a NULL argument (before any device work); nq == 0 is a no-op.
 */
int cwq_rank_scores_backward(cwq_index* idx, const float* q, int64_t nq, const float* grad_out, float* grad_q,
                             void* stream);

/*
 * Cross-entropy ranking loss over ALL sentence scores, its gradient, and the target's score
 * and rank, without a [nq*n_sent] array on either side of this call.  Replaces the loop of
 * FixedDocsRankingLoss.forward (src/training/cobweb_query_train.py:104-126:
 * cobweb_rank_scores -> CrossEntropyLoss(scores / temperature, label) per query) and the
 * per-query numbers of evaluate() (:213-304: the true document's score and its position in a
 * full argsort).
 *   q            device [nq*dim] fp32
 *   target       device [nq] int64 sentence ids (the reference's labels: columns of
 *                cobweb_rank_scores)
 *   temperature  finite, > 0
 *   loss         device [nq]: logsumexp_s(score[q][s] / T) - score[q][target[q]] / T over the
 *                sentences in the tree (the others score -inf and add nothing, as in torch);
 *                per query, not reduced
 *   grad_q       device [nq*dim]: d loss[q] / d q[q][:]; NULL: forward only (no backward pass)
 *   target_score device [nq] or NULL: the target's score, the bits cwq_rank_scores writes
 *   rank         device [nq] int64 or NULL: 1 + the number of sentences before the target in
 *                cwq_score_topk's order (higher score, then lower node index, then lower
 *                sentence id), so rank <= k exactly when cwq_score_topk(k) returns the target
 * A target outside [0, n_sent) or whose sentence is not in the tree: loss +inf, a zero grad_q
 * row, target_score -inf, rank -1 (torch: inf / NaN); the other queries are not affected.
 * No float atomics: identical from run to run, and a query's outputs do not depend on the
 * other queries of the call or on the workspace chunking.  CWQ_ERR_ARG before any device
 * work for a NULL idx / q / target / loss, nq < 0, or a temperature that is not finite and
 * > 0; nq == 0 is a no-op.  Keeps no state between calls.
 */
int cwq_rank_ce(cwq_index* idx, const float* q, int64_t nq, const int64_t* target, float temperature,
                float* loss, float* grad_q, float* target_score, int64_t* rank, void* stream);

/*
 * The three calls above under call-time level weights, with the gradient with respect to them.
 * The Fast score is linear in the level weights (score = (1/L) sum_depth w[depth] lp'(node));
 * an index bakes them in at creation, and these calls evaluate it under another vector
 * without a rebuild and return d/dw, so a schedule can be swept or learned against a fixed
 * index and written back once (a new index with the learned weights).
 *   level_w  device [n_w] fp32 on the index's device, read by the kernels only (no host read,
 *            no sync); a depth >= n_w weighs 1.0, as at index creation.  Any finite value of
 *            either sign; non-finite weights propagate as in torch.  NULL: the index's own
 *            weights -- the outputs are then exactly those of the calls above.
 *   n_w      0 <= n_w <= 64
 *   grad_w   device [nq*n_w] fp32 or NULL: cwq_rank_scores_backward_w: d(sum grad_out *
 *            scores[q])/dw per query; cwq_rank_ce_w: d loss[q]/dw.  Per query, not reduced;
 *            columns of levels deeper than the tree are 0; an invalid target gives a zero row.
 *            fp64 accumulation in a fixed order over fixed row ranges, no atomics: identical
 *            from run to run, for a query alone, in any batch and under workspace chunking.
 *   grad_q   as above; may be NULL in cwq_rank_scores_backward_w when grad_w is not.
 * With level_w given, the forward outputs and grad_q are bit for bit those of an index created
 * with these weights (as doubles).  The index is not modified.  CWQ_ERR_ARG before any device
 * work for n_w outside [0, 64] or a NULL required pointer.  Only these exact paths take
 * call-time weights: retrieval (cwq_score_topk and the filters) reads the baked ones.
 */
int cwq_rank_scores_w(cwq_index* idx, const float* q, int64_t nq, const float* level_w, int32_t n_w, float* out,
                      void* stream);
int cwq_rank_scores_backward_w(cwq_index* idx, const float* q, int64_t nq, const float* grad_out,
                               const float* level_w, int32_t n_w, float* grad_q, float* grad_w, void* stream);
int cwq_rank_ce_w(cwq_index* idx, const float* q, int64_t nq, const int64_t* target, float temperature,
                  const float* level_w, int32_t n_w, float* loss, float* grad_q, float* grad_w, float* target_score,
                  int64_t* rank, void* stream);

/*
 * Sparse differentiable scores (no reference counterpart: the reference scores every leaf,
 * CobwebWrapper.py:267-294): the Fast scores of a short list of sentences per
 * query, their backward, and the cross-entropy loss over the exact top-K plus the target.
 * All three validate their arguments before any device work (CWQ_ERR_ARG for a NULL required
 * pointer, nq < 0, m < 1, K < 1 or a temperature that is not finite and > 0), treat nq == 0 as
 * a no-op, run on `stream`, use no float atomics (every output is bit-identical from run to
 * run, and a query's outputs are the same alone, in any batch and under any workspace
 * chunking) and keep no state between calls.
 *
 * cwq_score_pairs
 *   ids     device [nq*m] int64: m sentence ids per query; duplicates allowed; any m >= 1
 *   scores  device [nq*m]: scores[q][j] = the Fast score of sentence ids[q][j] for query q, bit
 *           for bit the value cwq_rank_scores writes in that column; -inf for an id of -1, an
 *           id outside [0, n_sent) and a sentence that is in no node
 *
 * cwq_score_pairs_backward
 *   grad_scores  device [nq*m]: the upstream gradient of every score.  Entries whose score is
 *                -inf are never read (cwq_rank_scores_backward's rule); duplicates add
 *   grad_q       device [nq*dim]: d(sum_j grad_scores[q][j] * score(q, ids[q][j])) / dq
 *   Needs nothing from a forward call.  m <= 4096; above it CWQ_ERR_ARG (scatter the gradient
 *   into [nq*n_sent] and call cwq_rank_scores_backward).
 *
 * cwq_rank_ce_topk
 *   The candidate set C of a query is what cwq_score_topk(K) returns for it (its order, its tie
 *   rule, its scores) plus the target when it is not among them.  With T the temperature, m the
 *   largest candidate score, z = sum_C exp((s - m)/T) and s_K the lowest top-K score:
 *   loss         device [nq]: (m - s_target)/T + log z
 *   grad_q       device [nq*dim] or NULL (forward only): d loss / dq, through the sparse backward
 *                with g_j = (exp((s_j - m)/T)/z - [j = target]) / T; needs K + 1 <= 4096
 *   target_score device [nq] or NULL: the bits cwq_rank_scores gives
 *   rank         device [nq] int64 or NULL: the exact 1-based rank (cwq_rank_ce's) when the target
 *                is inside the top-K, otherwise K + 1 = "at least K + 1"
 *   tail_bound   device [nq] or NULL: a certified upper bound of cwq_rank_ce's loss minus this
 *                loss, log1p((n_tree - |C|) exp((s_K - m)/T) / z) with n_tree the sentences that
 *                are in the tree (every sentence outside C scores at most s_K); 0 when fewer
 *                than K sentences exist
 *   cand_ids     device [nq*K] int64 or NULL: the row cwq_score_topk returns
 *   A target outside [0, n_sent) or whose sentence is not in the tree: loss +inf, a zero grad_q
 *   row, target_score -inf, rank -1, tail_bound 0 (cwq_rank_ce's result); the other queries are
 *   not disturbed.  Any K >= 1 that cwq_score_topk accepts; K <= 64 is the hot form.
 */
int cwq_score_pairs(cwq_index* idx, const float* q, int64_t nq, const int64_t* ids, int32_t m, float* scores,
                    void* stream);
int cwq_score_pairs_backward(cwq_index* idx, const float* q, int64_t nq, const int64_t* ids, int32_t m,
                             const float* grad_scores, float* grad_q, void* stream);
int cwq_rank_ce_topk(cwq_index* idx, const float* q, int64_t nq, const int64_t* target, float temperature, int32_t K,
                     float* loss, float* grad_q, float* target_score, int64_t* rank, float* tail_bound,
                     int64_t* cand_ids, void* stream);

/*
 * Per-node Gaussian log-likelihood for every node in BFS order.
 *   full = 0: lp'(n) as CobwebWrapper.py:232-236 (no 2*pi term)
 *   full = 1: CobwebTorchNode.log_prob (CobwebTorchNode.py:100-104, with 2*pi)
 * out: device [nq*n_nodes] fp32.
 */
int cwq_node_logprob(cwq_index* idx, const float* q, int64_t nq, int32_t full, float* out, void* stream);

/*
 * Diagnostic (parity tests): the Fast path's internal path prefixes P (the level-
 * weighted sum of lp' along the path: the reference's sparse path matrix,
 * CobwebWrapper.py:145-180, restricted to ancestors) of every internal node by the
 * exact fp32 pass -> exact, and the rigorous bf16-MFMA bounds lo <= exact <= hi the
 * filter uses on hierarchical trees (NaN for nodes the filter does not read: with the
 * default path-sum bounds, internal nodes without isotropic leaf children).  All
 * device [nq][n_internal] fp32, internal nodes in BFS order; 1 <= nq <= 4096.
 * CWQ_ERR_ARG when the index keeps no bounds (flat tree, no isotropic leaf rows).
 */
int cwq_prefix_bounds(cwq_index* idx, const float* q, int64_t nq, float* lo, float* hi, float* exact, void* stream);

/*
 * "Cobweb Basic" best-first categorize (A4).  Replaces CobwebTorchTree.categorize
 * / _cobweb_categorize with retrieve_k=k (CobwebTorchTree.py:235-310) as called by
 * CobwebWrapper.cobweb_predict (CobwebWrapper.py:435-461).
 *   nodes     device [nq*k] int64: BFS indices of the retrieved nodes in pop order
 *             (-1 past n_found)
 *   n_found   device [nq] int32: number retrieved (< k where the reference raises
 *             IndexError: too few leaves, or max_nodes reached, :264-289)
 *   n_calls   device [nq] int64: log_prob evaluations the reference would make
 *             (may be NULL)
 * Heap ties: (-lp, parent lp, BFS index) -- the reference uses random() as the
 * third key.  The call synchronises `stream` (it may re-run hard queries).
 * Returns CWQ_OK also when some queries found < k nodes: callers check n_found
 * (the Python drop-in raises IndexError there, as the reference does).
 */
int cwq_categorize(cwq_index* idx, const float* q, int64_t nq, int32_t k, int64_t max_nodes, int64_t* nodes,
                   int32_t* n_found, int64_t* n_calls, void* stream);

/*
 * Device timing of the phases of the last cwq_score_topk call, measured with HIP
 * events recorded on the stream the kernels run on (enable first; timing mode
 * synchronises the stream once per query chunk).  Milliseconds:
 *   out[0] leaf rows (scan, or the whole filter pipeline)   out[1] internal-node pass
 *   out[2] merge + sentence expansion                        out[3] whole call
 *   out[4] number of leaf-row launches
 *   filter pipeline only: out[5] threshold sample pass (fgemm + select)
 *   out[6] the filter fgemm launches (sum)                  out[7] last bucket + exact rerank
 */
int cwq_set_timing(cwq_index* idx, int enable);
int cwq_last_timing(cwq_index* idx, float* out8);

/*
 * Isotropic-row strategy of cwq_score_topk (no reference counterpart: an execution
 * choice; results are identical either way).
 *   mode -1: automatic (default; env CWQ_FILTER=0/1 overrides): the bf16-MFMA
 *            candidate filter + exact rerank when k <= 64 and the index holds
 *            >= 16384 isotropic rows, the exact fp32 scan otherwise; an index on which
 *            >= 9 in 10 of its first >= 256 filtered queries had to be re-run exactly (the
 *            bounds too loose for its rows) stays on the exact scan from then on
 *   mode  0: always the exact fp32 scan      mode 1: the filter whenever k <= 64
 * Calls with nq <= 64 take the small-batch stream filter instead of the batch MFMA
 * filter (one HBM pass over the bf16 row panel; env CWQ_STREAM=0 disables it).
 * cwq_last_stats(out6): [queries served by the filter, of which re-run by the exact
 * scan (candidate list overflow / no threshold), filter used (0 exact scan, 1 batch
 * MFMA filter, 2 small-batch stream filter; + 256 when the stream filter's pass ran on
 * the int8 row panel; + 65536 per batch filter launch that ran on the int8 operands --
 * env CWQ_FG_I8: negative off, n >= 0 from filter phase n on), mean candidate records per query, mean
 * exact reranks per query, threshold-sample rows].
 * After cwq_categorize, cwq_last_stats reports instead: [queries, queries re-run with
 * every leaf row materialised (DENSE), queries re-run after a filter list overflow,
 * queries resolved by counting over the bottleneck order, queries resolved by the heap
 * replay, queries the two-level replay resolved after their list ended inside a
 * bottleneck tie].
 */
int cwq_set_filter(cwq_index* idx, int mode);
/*
 * cwq_score_topk with host memory on both sides: q (host [nq*dim]) in, ids (host [nq*k])
 * and scores (host [nq*k] or NULL) out; returns synchronized.  The reference harness's
 * timed call shape (benchmark_utils.py:801-805: cobweb_predict_fast on a numpy embedding,
 * CobwebWrapper.py:428-433 -> :210-265).  Same results as cwq_score_topk.
 */
int cwq_score_topk_host(cwq_index* idx, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                        void* stream);
/*
 * cwq_categorize with host memory on both sides: q (host [nq*dim]) in; nodes (host
 * [nq*k]), n_found (host [nq]) and n_calls (host [nq] or NULL) out; returns synchronized.
 * The reference harness's Basic call shape (benchmark_utils.py:580-581: cobweb_predict on a
 * numpy embedding, CobwebWrapper.py:435-461 -> CobwebTorchTree.py:235-289).  Same results
 * as cwq_categorize.
 */
int cwq_categorize_host(cwq_index* idx, const float* q, int64_t nq, int32_t k, int64_t max_nodes, int64_t* nodes,
                        int32_t* n_found, int64_t* n_calls, void* stream);

int cwq_last_stats(cwq_index* idx, int64_t* out6);

/*
 * Masked Fast top-k: cwq_score_topk restricted to an allowed sentence set (no reference
 * counterpart: the reference always ranks every sentence).  One mask per call,
 * shared by the call's queries.
 *
 * The result for a query is its full cwq_score_topk ranking (key descending, then lower node
 * index, then lower sentence id) with the sentences that are not allowed removed, cut to k:
 * ids and scores are that ranking's bit for bit.  When fewer than k allowed sentences are in
 * the tree the tail is -1 / -inf, as for k > n_sent.  A sentence that is not in the tree
 * (node_of_sentence -1) is never returned, whatever its bit.  Any k >= 1 is accepted.
 *
 * cwq_mask_create
 *   bits    device uint32 words, ceil(n_sent / 32) of them: bit (s % 32) of word (s / 32),
 *           least significant bit first, set = sentence s is allowed.  Copied: the caller
 *           may free it when the call returns (the call synchronises `stream`, as
 *           cwq_index_create does).
 *   n_sent  must equal the index's (CWQ_ERR_ARG otherwise)
 * A mask remembers the index it was built for by that index's serial number, not by its
 * address: cwq_score_topk_masked with another index -- also a new index at the old address
 * -- is CWQ_ERR_ARG with a message.  A mask holds no pointer into its index, so it may
 * outlive it, and the two may be destroyed in either order.  A mask is immutable after its
 * creation and may be shared by calls on different streams and threads.
 * cwq_mask_info(out4): [allowed sentences that are in the tree, live isotropic rows, live
 * anisotropic rows (a row is live when one of its sentences is allowed), device bytes].
 *
 * cwq_score_topk_masked: arguments as cwq_score_topk.  It takes one of three paths, with
 * identical results:
 *   1 over-fetch  cwq_score_topk's own work at some k' <= 64 into buffers of the handle, the
 *                 allowed entries kept in order; a query with fewer than min(k, allowed)
 *                 survivors is redone by path 2 (every allowed sentence outside the unmasked
 *                 top-k' ranks below all of it, so the survivors are a prefix of the answer)
 *   2 gathered    an exact fp32 scan of the live rows only, through the mask's row lists
 *   3 sort        k > 64: every row's exact key, the rows that are not live set to -inf, the
 *                 full sort of cwq_score_topk's k > 64 path, a masked expansion
 * For k <= 64 the choice follows the allowed fraction f: over-fetch when k' = ceil(2 k / f)
 * is at most 64 (calls of <= 64 queries) or 40 (larger calls, whose unmasked filter gets
 * expensive past that), else gathered.  Env CWQ_MASK_PATH, read per call: 0 / unset
 * automatic, 1 over-fetch first (k' = 64 below the rule's fraction), 2 gathered only.  The
 * choice never changes a result.  The call synchronises
 * `stream` on path 1 (it reads the per-query flags back).  A mask without a live row
 * returns all -1 / -inf without a scan.  CWQ_ERR_ARG before any device work for a NULL idx /
 * mask / q / ids or k <= 0; nq == 0 is a no-op.
 * cwq_last_mask_stats(out4): [path (1, 2, 3), k' (path 1, else 0), queries redone by the
 * gathered scan (path 1), live rows of the mask].  After path 1, cwq_last_stats describes
 * the unmasked call at k'.
 */
typedef struct cwq_mask cwq_mask;
int cwq_mask_create(cwq_index* idx, const uint32_t* bits, int64_t n_sent, void* stream, cwq_mask** out);
int cwq_mask_destroy(cwq_mask* m);
int cwq_mask_info(const cwq_mask* m, int64_t* out4);
int cwq_score_topk_masked(cwq_index* idx, const cwq_mask* m, const float* q, int64_t nq, int32_t k, int64_t* ids,
                          float* scores, void* stream);
int cwq_last_mask_stats(const cwq_index* idx, int64_t* out4);

/*
 * Per-query masks: one masked call over queries with different allowed sets.
 * Row i of the result is, bit for bit in ids and scores, what
 * cwq_score_topk_masked(idx, masks[mask_of_query[i]], q + i * dim, 1, k, ...) returns.
 *   masks          n_masks masks of this index; a mask may stand in several slots or be unused
 *   mask_of_query  HOST memory, nq entries in [0, n_masks): the plan is made on the host
 * For k <= 64 every mask that queries name is classed by cwq_score_topk_masked's rule at the
 * call's whole nq (CWQ_MASK_PATH forces all masks one way).
 *   - The over-fetch masks share one unmasked call per width k' in {16, 32, 40, 64} (a
 *     mask's k' rounded up; a call of <= 64 queries runs one width, its widest) and one
 *     read-back of the short flags.
 *   - The queries planned to the gathered scan and the short ones are staged sorted by mask
 *     and scanned by at most four kernel launches per workspace chunk (segment x form),
 *     however many masks the call names.
 *   - Queries of a mask without a live row are -1 / -inf and never scanned.
 *   - A mask with <= 64 queries that the rule over-fetches as a call of that size, but sends
 *     to the gathered scan at the whole nq (a batch caps k' at 40), runs as a single-mask
 *     call of its own inside this call.
 *   - The loop form: where the gathered scan's own work dwarfs the per-call cost saved (its
 *     planned row-queries at 14.4 G/s x 768 / DP above 4 x 0.3 ms x masks, constants fitted
 *     on flat 1M x 768), every mask runs as a single-mask call of its own.
 *     Stats [1], [4] and [5] then stay 0.
 * k > 64: the sort path per mask on its gathered queries.  When every query names the same
 * mask the call is cwq_score_topk_masked itself (same path, same cwq_last_mask_stats).
 * The rows are the same bits whichever way a mask runs.  Env CWQ_MASK_MULTI_FORM, read per
 * call: 0 / unset the rules, 1 grouped only, 2 loop form.
 * The call synchronises `stream`.
 * CWQ_ERR_ARG with a message, before any device work: a NULL idx / masks / mask_of_query, a
 * NULL q / ids at nq > 0, n_masks < 1, k <= 0, a NULL entry of masks, a mask built for
 * another index, an entry of mask_of_query outside [0, n_masks) (the message names the first
 * such query).  nq == 0 is a no-op.
 * cwq_last_mask_multi_stats(out8): [queries answered by the over-fetch leg, distinct
 * over-fetch widths run, queries the over-fetch left short (redone by the gathered scan),
 * queries planned straight to the gathered scan, gathered-scan kernel launches, gathered-scan
 * work items (workgroups), distinct masks referenced, queries through the k > 64 sort].
 * After a multi call cwq_last_mask_stats reports [4, the widest over-fetch width run (0:
 * none), queries left short, live rows summed over the distinct masks referenced].
 */
int cwq_score_topk_masked_multi(cwq_index* idx, const cwq_mask* const* masks, int32_t n_masks,
                                const int32_t* mask_of_query, const float* q, int64_t nq, int32_t k, int64_t* ids,
                                float* scores, void* stream);
int cwq_last_mask_multi_stats(const cwq_index* idx, int64_t* out8);

/*
 * Masked ranking loss (no reference counterpart): cwq_rank_ce and
 * cwq_rank_ce_topk over an allowed sentence set.  With A the sentences that the mask allows
 * and that are in the tree, and T the temperature:
 *   loss[q]  = logsumexp_{s in A}(score(q, s) / T) - score(q, target[q]) / T
 *   rank[q]  = 1 + the sentences of A before the target in cwq_score_topk's order (key
 *              descending, then lower node index, then lower sentence id): rank <= k exactly
 *              when cwq_score_topk_masked(k) returns the target
 *   target_score[q] = the bits cwq_rank_scores writes for the target
 * A target that is not in A (not allowed, out of range, or not in the tree) is handled as
 * cwq_rank_ce handles an invalid target: loss +inf, a zero grad_q row, target_score -inf,
 * rank -1, the other queries undisturbed.  A mask without a live row gives that for every
 * query, without a scan.  No float atomics: the outputs are bit-identical from run to run, and
 * a query's outputs are the same alone, in any batch and under any workspace chunking.
 *
 * cwq_rank_ce_masked: arguments as cwq_rank_ce plus the mask (grad_q, target_score and rank
 * may be NULL).  Two paths, chosen from the mask alone (never from nq):
 *   full      cwq_rank_ce's pipeline -- the exact scan and the backward stream over every
 *             row -- with each row's sentence count replaced by its allowed count (computed
 *             per call from the mask's bitset; the mask holds no counts)
 *   gathered  both streams over the mask's live rows only: the gathered exact scan writes
 *             the live rows' keys (the exact scan's bits) into key lines pre-filled with
 *             -inf, and the backward walks the mask's row lists
 * loss, target_score and rank are bit-identical between the paths (the [row]-indexed key and
 * coefficient arrays are dense on both); grad_q may differ by summation order.  The gathered
 * path is taken when the live rows are fewer than 0.55 of the leaf-class rows (fitted on flat
 * 1M x 768 and 100k x 768).  Env CWQ_MASK_CE_PATH, read per call: 0 / unset
 * automatic, 1 full, 2 gathered.  cwq_last_mask_stats then reports [path code 5 (full) or 6
 * (gathered), 0, 0, live rows of the mask].
 *
 * cwq_rank_ce_topk_masked: cwq_rank_ce_topk with the candidates from the masked retrieval.
 *   masks, n_masks, mask_of_query  as cwq_score_topk_masked_multi (mask_of_query: HOST
 *             memory, nq entries); mask_of_query may be NULL when n_masks == 1
 * C = the target plus what cwq_score_topk_masked(K) (several masks:
 * cwq_score_topk_masked_multi) returns; cand_ids is that row bit for bit;
 *   tail_bound = log1p((n_allowed(q) - |C|) exp((s_K - m) / T) / z)
 * with the query's own mask's allowed count; rank is exact inside the top-K, else K + 1.  Row
 * i of a call over several masks equals the single-mask call on query i alone, bit for bit in
 * every output.  The call synchronises `stream`.
 *
 * Both: CWQ_ERR_ARG with a message, before any device work, for a NULL idx / mask(s) / q /
 * target / loss, a mask of another index, nq < 0, K < 1, a temperature that is not finite or
 * not > 0, n_masks < 1, a NULL mask_of_query with n_masks != 1, an entry of mask_of_query
 * outside [0, n_masks), K + 1 > 4096 with grad_q.  nq == 0 is a no-op.
 */
int cwq_rank_ce_masked(cwq_index* idx, const cwq_mask* m, const float* q, int64_t nq, const int64_t* target,
                       float temperature, float* loss, float* grad_q, float* target_score, int64_t* rank,
                       void* stream);
int cwq_rank_ce_topk_masked(cwq_index* idx, const cwq_mask* const* masks, int32_t n_masks,
                            const int32_t* mask_of_query, const float* q, int64_t nq, const int64_t* target,
                            float temperature, int32_t K, float* loss, float* grad_q, float* target_score,
                            int64_t* rank, float* tail_bound, int64_t* cand_ids, void* stream);

/*
 * Group pruning of the Fast query (clustered trees whose rows are
 * group-centred, every level weight >= 0): per (query, depth-1 group) a certified upper
 * bound of every key in the group; the exact internal pass runs for each query's best group
 * and then only for the groups whose bound reaches the filter's first threshold.  Results
 * are unchanged (bit-identical to the exact scan); CWQ_GROUP_PRUNE=0 turns it off (at index
 * creation: never built; per call: not used).  Replaces no reference call: the reference
 * evaluates every node (CobwebWrapper.py:222-241).
 * cwq_last_prune_stats(out4): [pruning available on this index, queries of the last Fast
 * call's pruned chunk (0: not pruned), its stage-B (query, group) pairs, groups].
 */
int cwq_last_prune_stats(cwq_index* idx, int64_t* out4);

/*
 * Sequential Welford statistics of row groups (synthetic-tree builder).
 * For group g, folds rows X[order[group_ptr[g]] .. order[group_ptr[g+1]-1]] in
 * that order with exactly the fp32 op sequence of CobwebTorchNode.increment_counts
 * (CobwebTorchNode.py:57-68: count += 1; delta = x - mean; mean += delta / count;
 * meanSq += delta * (x - mean)), so a synthesised internal node carries the stats
 * the reference's ifit would accumulate for those inserts.
 *   X [n_rows*dim], order [n_order], group_ptr [n_groups+1]: device
 *   count [n_groups], mean/meanSq [n_groups*dim]: device outputs
 */
int cwq_welford_groups(const float* X, int64_t n_rows, int32_t dim, const int64_t* order, const int64_t* group_ptr,
                       int64_t n_groups, float* count, float* mean, float* meanSq, void* stream);

/*
 * Incremental fit (ifit) support: category-utility scoring on the GPU (add path,
 * CobwebTorchTree.cobweb, CobwebTorchTree.py:143-233).  Node statistics live in a
 * caller-owned device pool: count[cap], mean[cap*dim], meanSq[cap*dim] (slot = row).
 *
 * cwq_fit_kl: out[j] = compute_score(cand_j, ref_j) = KL(cand || ref)
 *   (CobwebTorchTree.py:344-364, use_info=True, use_kl=True) for jobs[4*j..4*j+3] =
 *   {cand_type, n1, n2, ref_type}:
 *     cand_type 0: node n1                    (CobwebTorchNode.mean_var, :211-212)
 *               1: node n1 with x inserted    (mean_var_insert, :214-222)
 *               2: new leaf from x            (mean_var_new, :204-209)
 *               3: merge(n1, n2) with x       (mean_var_merge, :224-239)
 *     ref_type  0: parent p_slot; 1: parent with x inserted.
 *   x, jobs, out: device.  Asynchronous on `stream`.
 */
int cwq_fit_kl(const float* count, const float* mean, const float* meanSq, int32_t dim, const float* x,
               float prior_var, int32_t p_slot, const int32_t* jobs, int32_t n_jobs, float* out, void* stream);

/*
 * cwq_fit_node_op: one node update in the pool, same fp32 op order as the reference:
 *   op 0 increment_counts(dst, x)           (CobwebTorchNode.py:57-68)
 *   op 1 update_counts_from_node(dst, src)  (:70-85; merge and the copy constructor)
 *   op 2 zero(dst)                          (a fresh node)
 *   op 3 *flag = is_exact_match(dst, x)     (:652-666, torch.isclose defaults)
 */
int cwq_fit_node_op(int32_t op, float* count, float* mean, float* meanSq, int32_t dim, int32_t dst, int32_t src,
                    const float* x, int32_t* flag, void* stream);

/*
 * Device-resident incremental fit (F1): CobwebTorchTree.cobweb's insert loop
 * (CobwebTorchTree.py:143-233; CobwebTorchNode.py:57-85, 374-666) run entirely on the
 * GPU -- the tree (statistics, parent links, ordered child lists) in device memory, one
 * master workgroup inserting the rows in order, every decision on the device, the
 * reference's random() draws from Python's MT19937 stream run on the device; a level with
 * many children (>= CWQ_FIT_FORK_MIN, default 64) has its KL terms computed by helper
 * workgroups on every CU (CWQ_FIT_HELPERS, default CUs - 1; 0 = one workgroup).  Builds the
 * same trees as the host-driven cwq_fit_kl / cwq_fit_node_op path (fit.py).  dim <= 1024.
 * Errors: CWQ_ERR_OOM only for a node pool / child arena that cannot be allocated or
 * runs out inside an insert (fit.py then continues on the host fitter); a chip-wide KL
 * pass that did not complete is CWQ_ERR_HIP (fit.py raises).
 *   cwq_fit_create   a handle with room for cap_nodes nodes
 *   cwq_fit_load     the tree in slots 0..n_nodes-1: parent (host, -1 at the root),
 *                    children in list order as CSR (host child_ptr [n+1], child_idx),
 *                    count / mean / meanSq (host, [n], [n*dim]); mt_state (host [625]) =
 *                    Python's random.getstate()[1] (624 words + index)
 *   cwq_fit_insert   X (device [n*dim]): the rows inserted in order; leaf_out (device
 *                    [n] int32) = the slot of the node each row ended in (ifit's return
 *                    value).  info (host int64[4]) = {rows done, random() draws, status,
 *                    slots in use}; status 1: the node pool / child arena needs room --
 *                    export, load into a larger handle and insert the remaining rows
 *   cwq_fit_export   out2 = {slots in use, root}; parent (-2: a node a split removed),
 *                    child CSR, count, mean, meanSq (host, [cap] / [cap*dim]) and the
 *                    random() state after the draws (host [625])
 *   cwq_mt19937_draw n draws of Python's random.random() from state625 (host; updates it)
 *   cwq_mt19937_words n 32-bit outputs (Python's getrandbits(32)) from state625 through the
 *                    chain-form twist the device's parallel generator runs (host; updates it)
 *   cwq_mt19937_skip  advance state625 past nwords 32-bit outputs without producing them
 *                    (host; updates it): the Basic query's random() advance -- one random()
 *                    = 2 words per heap push and retrieval (CobwebTorchTree.py:243,268,285),
 *                    replacing getrandbits(64 n) (CobwebWrapper.cobweb_predict, wrapper.py)
 */
typedef struct cwq_fit cwq_fit;
int cwq_fit_create(int device, int32_t dim, float prior_var, int32_t cap_nodes, cwq_fit** out);
int cwq_fit_destroy(cwq_fit* h);
int cwq_fit_load(cwq_fit* h, int32_t n_nodes, int32_t root, const int32_t* parent, const int32_t* child_ptr,
                 const int32_t* child_idx, const float* count, const float* mean, const float* meanSq,
                 const uint32_t* mt_state, void* stream);
int cwq_fit_insert(cwq_fit* h, const float* X, int64_t n, int32_t* leaf_out, int64_t* info, void* stream);
int cwq_fit_export(cwq_fit* h, int32_t* out2, int32_t* parent, int32_t* child_ptr, int32_t* child_idx, float* count,
                   float* mean, float* meanSq, uint32_t* mt_state, void* stream);
const char* cwq_fit_last_error(void);
int cwq_mt19937_draw(uint32_t* state625, int64_t n, double* out);
int cwq_mt19937_words(uint32_t* state625, int64_t n, uint32_t* out);
int cwq_mt19937_skip(uint32_t* state625, int64_t nwords);

/*
 * The device-resident tree between an add and the next query: the query index built
 * straight from a cwq_fit handle, the handle grown in place, and the random() state moved
 * on its own.  Replaces, per CobwebWrapper.add_sentences -> cobweb_predict* cycle
 * (CobwebWrapper.py:52-89), the host passes over every node: the BFS flatten and
 * compute_var of build_prediction_index (CobwebWrapper.py:107-203, CobwebTorchTree.py:336-342)
 * and the export / reload of the whole tree around each insert batch.  No [n_nodes*dim]
 * float array crosses PCIe.  All calls validate their arguments before any device work
 * (CWQ_ERR_ARG, message in cwq_fit_last_error; cwq_index_create_from_fit also sets
 * cwq_last_error), and are ordered on `stream`.
 *
 *   cwq_fit_flatten   the live tree in BFS numbering -- exactly CobwebWrapper's (root 0, a
 *                     node's children consecutive in child-list order, levels in order;
 *                     slots a split removed get no number) -- as device arrays owned by the
 *                     returned object: mean [n_nodes*dim], count [n_nodes], the variances meanSq / count +
 *                     prior_var (numpy float32 bits; prior_var for an empty node) in
 *                     cwq_index_create_cv's compact form (var_row [n_nodes], an_nodes [n_an]
 *                     ascending = the nodes whose dim variances are not all the same bits,
 *                     an_var [n_an*dim]), parent [n_nodes] int64, slot_of_node [n_nodes] int32
 *                     and node_of_sentence [n_sent] int64 from slot_of_sentence (device
 *                     [n_sent] int32, the slot holding each sentence; -1 or a slot that is
 *                     not in the tree: -1).  Trees of up to 64 levels below the root; deeper
 *                     ones are CWQ_ERR_ARG.  One 8-byte readback per level.
 *   cwq_fit_flat_info o[8] = {n_nodes, n_an, n_sent, dim, levels below the root, slots in
 *                     use, device bytes held, 0}
 *   cwq_fit_flat_copy device-to-device copies into the caller's arrays (NULL: skipped)
 *   cwq_index_create_from_fit  flatten, download parent and node_of_sentence (8 B per node
 *                     and per sentence), build the index from the device-resident mean and
 *                     compact variances (the index of cwq_index_create_cv on the same
 *                     arrays), free the temporaries
 *   cwq_fit_grow      the pool and the child arena re-allocated at new_cap_nodes (> the
 *                     capacity) device to device, slot numbers unchanged, child lists
 *                     re-packed at max(4, 2 * length) as cwq_fit_load lays them out; control
 *                     words, log-variance cache and random() state kept.  Answers a status-1
 *                     return of cwq_fit_insert without export and reload.  CWQ_ERR_OOM: the new
 *                     pool cannot be allocated; the handle is unchanged and usable
 *   cwq_fit_set_rng / cwq_fit_get_rng   upload / download the handle's random() state (host
 *                     [625]: random.getstate()[1]), for the one global stream that ifit and
 *                     categorize share (CobwebTorchTree.py:243,268,285)
 *   cwq_fit_rewind    the next cwq_fit_insert starts at row 0 of its X again (a new batch into
 *                     the same handle)
 *   cwq_fit_info      o[8] = {capacity, slots in use, root slot, slots removed by splits, arena
 *                     top, arena capacity, rows done, random() draws}
 */
typedef struct cwq_fit_flat cwq_fit_flat;
int cwq_fit_flatten(cwq_fit* h, const int32_t* slot_of_sentence, int64_t n_sent, void* stream, cwq_fit_flat** out);
int cwq_fit_flat_info(const cwq_fit_flat* flat, int64_t* out8);
int cwq_fit_flat_copy(const cwq_fit_flat* flat, float* mean, float* count, float* var_row, int64_t* an_nodes, float* an_var,
                      int64_t* parent, int64_t* node_of_sentence, int32_t* slot_of_node, void* stream);
int cwq_fit_flat_destroy(cwq_fit_flat* flat);
int cwq_index_create_from_fit(cwq_fit* h, const int32_t* slot_of_sentence, int64_t n_sent, const double* level_w,
                              int32_t n_w, void* stream, cwq_index** out);
int cwq_fit_grow(cwq_fit* h, int32_t new_cap_nodes, void* stream);
int cwq_fit_set_rng(cwq_fit* h, const uint32_t* state625, void* stream);
int cwq_fit_get_rng(cwq_fit* h, uint32_t* state625, void* stream);
int cwq_fit_rewind(cwq_fit* h, void* stream);
int cwq_fit_info(cwq_fit* h, int64_t* out8, void* stream);

/*
 * PCA + ICA whitening transform (F4).  Replaces PCAICAWhiteningModel.transform
 * (src/whitening/pca_ica.py:30-51), the embedding normalisation of the "PCA + ICA"
 * benchmark rows and of config C5:
 *   x_pca = ((X - mean) @ comps^T) / denom,   out = x_pca @ unmix^T   (unmix != NULL)
 *                                             out = x_pca            (unmix == NULL, is_ica=False)
 *   X      device [n*d_in] fp32          mean   device [d_in]
 *   comps  device [d_pca*d_in]           denom  device [d_pca] = sqrt(explained_var + eps),
 *                                               computed by the caller in fp32 like numpy
 *   unmix  device [d_out*d_pca] or NULL  work   device [n*d_pca] scratch (when unmix)
 *   out    device [n*d_out] (or [n*d_pca])
 * fp32 MFMA GEMMs; results equal numpy's fp32 up to the dot-product summation order.
 */
int cwq_whiten(const float* X, int64_t n, int32_t d_in, const float* mean, const float* comps, int32_t d_pca,
               const float* denom, const float* unmix, int32_t d_out, float* out, float* work, void* stream);

/*
 * Whitening fits on the GPU: the row-proportional passes of PCAICAWhiteningModel.fit
 * (src/whitening/pca_ica.py:55-76: the mean :59, PCA :63-66, FastICA :72-74),
 * ZCAWhiteningModel.fit (src/whitening/zca.py:32-51: mean :36, np.cov :40) and
 * PCAZCAWhiteningModel.fit (src/whitening/pca_zca.py:47-60).  The small d x d algebra
 * (eigh, FastICA's symmetric decorrelation) stays with the caller, in fp64.
 *
 * All three are handle-less and stream-ordered, accumulate INTO their fp64 outputs (the
 * caller zeroes them and may call repeatedly over row chunks), take scratch from the
 * caller (`*_work_bytes`; -1 for a bad shape) and use no atomics: rows are cut into
 * fixed slabs (cwq_whitenfit_slab() rows; 128-row tiles for gsum), each slab is summed
 * on its own (the GEMMs in fp32 on v_mfma_f32_32x32x2_f32) and the slab partials are
 * added in slab order in fp64, so results are bit-identical from run to run on any
 * device.  Dimensions are in [1, 1024]; n == 0 is a no-op; bad arguments return
 * CWQ_ERR_ARG before any device work.
 *
 *   cwq_col_sums : acc[j] += sum_r X[r][j]                       X [n*d] fp32, acc [d] fp64
 *   cwq_gram_acc : acc[i][j] += sum_r (A[r][i] - ctr_a[i]) (B[r][j] - ctr_b[j])
 *                  A [n*da], B [n*db] fp32; ctr_a [da], ctr_b [db] or NULL; acc [da*db] fp64.
 *                  With A == B, ctr_a == ctr_b only the upper tiles are computed and mirrored.
 *   cwq_ica_g    : G = tanh(X1 W^T) [n*p] fp32, gsum[j] += sum_r (1 - G[r][j]^2) [p] fp64
 *                  (FastICA's logcosh g and g', sklearn _fastica.py _logcosh with alpha = 1)
 *                  X1 [n*p], W [p*p] fp32.
 */
int cwq_whitenfit_slab(void);
int64_t cwq_col_sums_work_bytes(int64_t n, int32_t d);
int64_t cwq_gram_acc_work_bytes(int64_t n, int32_t da, int32_t db);
int64_t cwq_ica_g_work_bytes(int64_t n, int32_t p);
int cwq_col_sums(const float* X, int64_t n, int32_t d, double* acc, void* work, void* stream);
int cwq_gram_acc(const float* A, const float* B, int64_t n, int32_t da, int32_t db, const float* ctr_a,
                 const float* ctr_b, double* acc, void* work, void* stream);
int cwq_ica_g(const float* X1, int64_t n, int32_t p, const float* W, float* G, double* gsum, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COBWEB_QUERY_H */
