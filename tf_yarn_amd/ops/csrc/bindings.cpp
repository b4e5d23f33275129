// Python bindings for the tf_yarn_amd MI355X kernel library.
#include <torch/extension.h>
#include <string>
#include <tuple>
#include <variant>
#include <vector>

// fused_optimizers.hip
void fused_sgd(torch::Tensor param, torch::Tensor grad,
               c10::optional<torch::Tensor> momentum_buf,
               c10::optional<torch::Tensor> param_bf16,
               double lr, double momentum, double dampening,
               double weight_decay, bool nesterov, bool first_step,
               double grad_scale);
void fused_sgd_mt(std::vector<torch::Tensor> params,
                  std::vector<torch::Tensor> grads,
                  std::vector<torch::Tensor> momentum_bufs,
                  std::vector<torch::Tensor> params_bf16,
                  double lr, double momentum, double dampening,
                  double weight_decay, bool nesterov, bool first_step,
                  double grad_scale);
void fused_adam(torch::Tensor param, torch::Tensor grad,
                torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                c10::optional<torch::Tensor> param_bf16,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, bool adamw, int64_t step,
                double grad_scale);
void fused_adagrad(torch::Tensor param, torch::Tensor grad,
                   torch::Tensor state_sum, double lr, double eps,
                   double weight_decay, double grad_scale);
void fused_ftrl(torch::Tensor param, torch::Tensor grad,
                torch::Tensor accum, torch::Tensor linear, double lr,
                double l1, double l2, double grad_scale);
void fused_adadelta(torch::Tensor param, torch::Tensor grad,
                    torch::Tensor square_avg, torch::Tensor acc_delta,
                    double lr, double rho, double eps, double weight_decay,
                    double grad_scale);

// embedding.hip
torch::Tensor emb_fwd(torch::Tensor table, torch::Tensor ids, bool out_bf16);
void emb_bwd_sgd(torch::Tensor table, torch::Tensor ids, torch::Tensor grad,
                 double lr, double scale);
void emb_bwd_sgd_sorted(torch::Tensor table, torch::Tensor sorted_ids,
                        torch::Tensor grad, double lr, double scale);
void emb_bwd_dense(torch::Tensor grad_table, torch::Tensor ids,
                   torch::Tensor grad, double scale);
void emb_bwd_sgd_fused_wide_offs(torch::Tensor table,
                                 torch::Tensor wide_table, torch::Tensor ids,
                                 torch::Tensor grad, torch::Tensor gw,
                                 double lr, double scale,
                                 c10::optional<torch::Tensor> offsets);
bool emb_lookup_fused_ok(int64_t dim, int64_t n_features, int64_t n_dense,
                         int64_t col_offset, int64_t out_cols);
torch::Tensor emb_lookup_fused(torch::Tensor table, torch::Tensor wide_table,
                               torch::Tensor ids, torch::Tensor offsets,
                               c10::optional<torch::Tensor> dense,
                               torch::Tensor out, int64_t col_offset);

torch::Tensor emb_gather_sum(torch::Tensor table, torch::Tensor ids,
                             int64_t batch, bool out_bf16);
void emb_fwd_into(torch::Tensor table, torch::Tensor ids,
                  torch::Tensor out, int64_t col_offset);
void emb_scatter_sum(torch::Tensor table, torch::Tensor ids,
                     torch::Tensor grad, double alpha);

// embedding_bag.hip
std::vector<torch::Tensor> emb_bag_fwd(
    torch::Tensor table, torch::Tensor ids, torch::Tensor bag_offsets,
    int64_t n_features, c10::optional<torch::Tensor> offsets,
    c10::optional<torch::Tensor> weights, const std::string& combiner,
    torch::Tensor out, int64_t col_offset);
torch::Tensor emb_bag_bwd_rows(torch::Tensor grad_out,
                               torch::Tensor bag_offsets,
                               torch::Tensor bag_scale, int64_t dim,
                               int64_t n_features, int64_t nnz,
                               c10::optional<torch::Tensor> weights,
                               int64_t col_offset);

// sparse_adagrad.hip
// one table's side of a stateful sparse update: (rule name, table, state
// tensors, accumulator, gradient or None, lr, eps, l1, l2); a lazy_adam
// side carries (beta1, beta2, step) after them
using SparseSide9 = std::tuple<std::string, torch::Tensor,
                               std::vector<torch::Tensor>, torch::Tensor,
                               c10::optional<torch::Tensor>, double, double,
                               double, double>;
using SparseSide12 = std::tuple<std::string, torch::Tensor,
                                std::vector<torch::Tensor>, torch::Tensor,
                                c10::optional<torch::Tensor>, double, double,
                                double, double, double, double, int64_t>;
using SparseSide = std::variant<SparseSide9, SparseSide12>;
void emb_bwd_sparse(c10::optional<SparseSide> deep,
                    c10::optional<SparseSide> wide, torch::Tensor stamp,
                    torch::Tensor ids, int64_t epoch, double scale);
bool sparse_pair_fused_ok(const std::string& deep_rule,
                          const std::string& wide_rule, int64_t dim);
// binned_scatter.hip
py::dict binned_layout();
std::vector<torch::Tensor> binned_permutation(torch::Tensor ids,
                                              int64_t n_rows,
                                              int64_t region_bits);
void emb_bwd_sgd_binned(torch::Tensor table, torch::Tensor ids,
                        torch::Tensor grad, double lr, double scale,
                        torch::Tensor order, torch::Tensor starts);
void emb_scatter_sum_binned(torch::Tensor table, torch::Tensor ids,
                            torch::Tensor grad, int64_t g_div,
                            double alpha, torch::Tensor order,
                            torch::Tensor starts);

// elementwise.hip
torch::Tensor bias_relu_fwd(torch::Tensor x, torch::Tensor bias);
torch::Tensor bias_relu_bwd(torch::Tensor dy, torch::Tensor y);
std::vector<torch::Tensor> bias_relu_bwd_db(torch::Tensor dy,
                                            torch::Tensor y,
                                            bool dbias_bf16);
std::vector<torch::Tensor> head_relu_bwd_db(torch::Tensor dl,
                                            torch::Tensor w_head,
                                            torch::Tensor y,
                                            bool dbias_bf16);
std::vector<torch::Tensor> head_relu_bwd_grads(torch::Tensor dl,
                                               torch::Tensor w_head,
                                               torch::Tensor y,
                                               bool out_bf16);
torch::Tensor reduce_splitk(torch::Tensor part, bool out_bf16);
torch::Tensor reduce_tall(torch::Tensor part, bool out_bf16,
                          int64_t quad_lanes);

// lt_linear.hip
torch::Tensor lt_linear(torch::Tensor x, torch::Tensor w,
                        c10::optional<torch::Tensor> bias, bool relu);
torch::Tensor col_reduce_dot(torch::Tensor x, torch::Tensor dy);
std::vector<torch::Tensor> col_reduce_dot_sum(torch::Tensor x,
                                              torch::Tensor dy,
                                              bool out_bf16);
torch::Tensor row_dot(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> bias);
std::vector<torch::Tensor> bce_head_fwd(torch::Tensor deep,
                                        torch::Tensor wide,
                                        torch::Tensor dhead,
                                        torch::Tensor labels);
torch::Tensor bce_head_bwd(torch::Tensor sig, torch::Tensor labels,
                           torch::Tensor g);

// wgrad.hip
torch::Tensor wgrad_nt128(torch::Tensor dy, torch::Tensor x,
                          int64_t splitk, bool out_bf16,
                          c10::optional<bool> regstage);
torch::Tensor wgrad_nt256(torch::Tensor dy, torch::Tensor x,
                          int64_t splitk, bool out_bf16,
                          c10::optional<bool> regstage);
py::dict wgrad_glds_layout();
void convert_scaled(torch::Tensor src, torch::Tensor dst, double scale);

// gemm_bt.hip
torch::Tensor gemm_bt(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> bias, bool relu);

// dgrad_drelu.hip
std::vector<torch::Tensor> dgrad_drelu(torch::Tensor dz_next, torch::Tensor w,
                                       torch::Tensor y, bool dbias_bf16);

// eval_metrics.hip
void binary_eval_update(torch::Tensor logits, torch::Tensor labels,
                        torch::Tensor hist, torch::Tensor counts,
                        torch::Tensor sums);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "tf_yarn_amd MI355X (gfx950) HIP kernels";
  m.def("fused_sgd", &fused_sgd, "Fused SGD(+momentum) step");
  m.def("fused_sgd_mt", &fused_sgd_mt,
        "Multi-tensor fused SGD (one launch per <=24 tensors)");
  m.def("fused_adam", &fused_adam, "Fused Adam/AdamW step");
  m.def("fused_adagrad", &fused_adagrad, "Fused Adagrad step");
  m.def("fused_adadelta", &fused_adadelta, "Fused Adadelta step");
  m.def("emb_fwd", &emb_fwd, "Fused multi-table embedding gather");
  m.def("emb_bwd_sgd", &emb_bwd_sgd,
        "Fused sparse embedding grad scatter + SGD update");
  m.def("emb_bwd_sgd_sorted", &emb_bwd_sgd_sorted,
        "Atomic-free segmented scatter+SGD over SORTED ids");
  m.def("emb_bwd_sgd_fused_wide", &emb_bwd_sgd_fused_wide_offs,
        "Fused deep scatter+SGD + wide scalar scatter (shared ids; with "
        "offsets, raw [batch, features] ids)",
        py::arg("table"), py::arg("wide_table"), py::arg("ids"),
        py::arg("grad"), py::arg("gw"), py::arg("lr"), py::arg("scale"),
        py::arg("offsets") = py::none());
  m.def("emb_lookup_fused_ok", &emb_lookup_fused_ok,
        "Whether emb_lookup_fused covers (dim, features, n_dense, "
        "col_offset, out_cols)");
  m.def("emb_lookup_fused", &emb_lookup_fused,
        "Offset add + deep gather into a slice + wide gather-sum + dense/"
        "pad columns in one kernel (returns the wide sums)",
        py::arg("table"), py::arg("wide_table"), py::arg("ids"),
        py::arg("offsets"), py::arg("dense"), py::arg("out"),
        py::arg("col_offset"));
  m.def("emb_bag_fwd", &emb_bag_fwd,
        "Pooled multi-hot lookup from CSR bags into a column slice of out; "
        "returns (bag_scale, flat_ids)",
        py::arg("table"), py::arg("ids"), py::arg("bag_offsets"),
        py::arg("n_features"), py::arg("offsets"), py::arg("weights"),
        py::arg("combiner"), py::arg("out"), py::arg("col_offset"));
  m.def("emb_bag_bwd_rows", &emb_bag_bwd_rows,
        "Pooled gradients -> per-entry update rows [nnz, dim]",
        py::arg("grad_out"), py::arg("bag_offsets"), py::arg("bag_scale"),
        py::arg("dim"), py::arg("n_features"), py::arg("nnz"),
        py::arg("weights"), py::arg("col_offset"));
  m.def("emb_bwd_dense", &emb_bwd_dense,
        "Sparse embedding grad scatter into dense grad table");
  m.def("emb_bwd_sparse", &emb_bwd_sparse,
        "Stateful sparse update (adagrad, ftrl, rowwise_adagrad, lazy_adam) "
        "of a deep "
        "side, a wide side or both from shared ids: atomic accumulate + "
        "once-per-row claim/apply; sides without gradients run the apply "
        "alone on their accumulators",
        py::arg("deep"), py::arg("wide"), py::arg("stamp"), py::arg("ids"),
        py::arg("epoch"), py::arg("scale"));
  m.def("sparse_pair_fused_ok", &sparse_pair_fused_ok,
        "Whether emb_bwd_sparse has a fused deep+wide kernel for (deep rule, "
        "wide rule, deep dim)");
  m.def("fused_ftrl", &fused_ftrl, "Fused dense FTRL-proximal step");
  m.def("bias_relu_fwd", &bias_relu_fwd, "Fused bias+ReLU forward");
  m.def("bias_relu_bwd", &bias_relu_bwd, "Fused ReLU backward");
  m.def("lt_linear", &lt_linear,
        "hipBLASLt linear with fused bias(+ReLU) epilogue",
        py::arg("x"), py::arg("w"), py::arg("bias") = py::none(),
        py::arg("relu") = false);
  m.def("reduce_splitk", &reduce_splitk,
        "Split-K partial reduction with fused output cast",
        py::arg("part"), py::arg("out_bf16") = false);
  m.def("reduce_tall", &reduce_tall,
        "reduce_splitk's tall-slab kernel with 1 or 4 quad lanes per block",
        py::arg("part"), py::arg("out_bf16") = false,
        py::arg("quad_lanes") = 1);
  m.def("wgrad_nt128", &wgrad_nt128,
        "Split-K MFMA weight gradient dW = dy^T @ x (bf16 in), 128x128 tiles; "
        "regstage: True = register-staged k-loop, False = LDS-DMA staging "
        "with transposed LDS reads, None = this tile's measured default",
        py::arg("dy"), py::arg("x"), py::arg("splitk"),
        py::arg("out_bf16") = false, py::arg("regstage") = py::none());
  m.def("wgrad_nt256", &wgrad_nt256,
        "Split-K MFMA weight gradient dW = dy^T @ x (bf16 in), 256x256 tiles; "
        "regstage: True = register-staged k-loop, False = LDS-DMA staging "
        "with transposed LDS reads, None = this tile's measured default",
        py::arg("dy"), py::arg("x"), py::arg("splitk"),
        py::arg("out_bf16") = false, py::arg("regstage") = py::none());
  m.def("wgrad_glds_layout", &wgrad_glds_layout,
        "Constants and image table of the wgrad kernels' LDS-DMA staging");
  m.def("col_reduce_dot", &col_reduce_dot,
        "dw[m] = sum_b dy[b] * x[b,m] (single-logit head wgrad)");
  m.def("col_reduce_dot_sum", &col_reduce_dot_sum,
        "col_reduce_dot plus db = sum_b dy[b] from the same pass "
        "(returns [dw, db])",
        py::arg("x"), py::arg("dy"), py::arg("out_bf16") = false);
  m.def("row_dot", &row_dot,
        "y[b] = x[b].w + bias (single-logit head forward GEMV)");
  m.def("bce_head_fwd", &bce_head_fwd,
        "Fused 3-part logit sum + stable BCEWithLogits (loss, sigmoid)");
  m.def("bce_head_bwd", &bce_head_bwd,
        "dlogit = (sigmoid - label) * upstream grad");
  m.def("bias_relu_bwd_db", &bias_relu_bwd_db,
        "Fused ReLU backward + dbias reduction (returns [dx, dbias])",
        py::arg("dy"), py::arg("y"), py::arg("dbias_bf16") = false);
  m.def("head_relu_bwd_db", &head_relu_bwd_db,
        "ReLU backward + dbias of the layer under a single-logit head, from "
        "dl and w_head (no outer product; returns [dz, dbias])",
        py::arg("dl"), py::arg("w_head"), py::arg("y"),
        py::arg("dbias_bf16") = false);
  m.def("head_relu_bwd_grads", &head_relu_bwd_grads,
        "head_relu_bwd_db plus the head's own dw and db from the same pass "
        "(returns [dz, dbias, dw_head, db_head])",
        py::arg("dl"), py::arg("w_head"), py::arg("y"),
        py::arg("out_bf16") = false);
  m.def("emb_fwd_into", &emb_fwd_into,
        "Embedding gather into a slice of a larger 2D buffer");
  m.def("emb_gather_sum", &emb_gather_sum,
        "Wide-part gather-sum: out[b] = sum_f table[ids[b,f]]");
  m.def("binned_layout", &binned_layout,
        "Layout constants of the binned scatter (hash capacities, probe "
        "limit, hash threshold, launch shapes)");
  m.def("binned_permutation", &binned_permutation,
        "Region-binned permutation of sparse update indices");
  m.def("emb_bwd_sgd_binned", &emb_bwd_sgd_binned,
        "Binned LDS-dedup scatter+SGD (deep tables, dim=16)");
  m.def("emb_scatter_sum_binned", &emb_scatter_sum_binned,
        "Binned LDS-dedup scatter-add (scalar wide tables)");
  m.def("emb_scatter_sum", &emb_scatter_sum,
        "Wide-part scatter: table[ids[b,f]] += alpha * g[b]");
  m.def("convert_scaled", &convert_scaled, "Scaled bf16<->fp32 convert");
  m.def("gemm_bt", &gemm_bt,
        "C = A @ B^T (both K-major bf16) with fused bias+ReLU epilogue");
  m.def("dgrad_drelu", &dgrad_drelu,
        "Hidden-layer dgrad dz_next @ w with the ReLU backward of the layer "
        "below and its dbias in the epilogue (returns [dz, dbias])",
        py::arg("dz_next"), py::arg("w"), py::arg("y"),
        py::arg("dbias_bf16") = false);
  m.def("binary_eval_update", &binary_eval_update,
        "Fold a batch of (logit, label) into the streaming binary eval "
        "state: score histogram [2, 4096], counts (n_valid, n_nan, tp, fp), "
        "per-slot fp64 (loss, sigmoid) sums [256, 2]",
        py::arg("logits"), py::arg("labels"), py::arg("hist"),
        py::arg("counts"), py::arg("sums"));
}
