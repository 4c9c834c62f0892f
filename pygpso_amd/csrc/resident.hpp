// What a context's device buffers currently hold.  Host side only; api.hip is the one file that includes this.  The buffers
// only grow and keep their old bytes: this record alone says which of them mean something.  Its members are written by
// the transitions below and nowhere else.  DESIGN.md, "What is resident": which entry point runs which transition, and
// where two of them differ on purpose.
#pragma once
#include <cstdint>
#include <utility>

#include "../../include/gpso_hip.h"

namespace gpso {

// the resident posterior: none, or where it came from
enum class Post { None, Fitted /* gpso_fit_eval, gpso_append */, Installed /* gpso_set_posterior */, Adopted /* a hand-off */,
                  Vgp, Sgpr, Svgp /* the variational predictives; the sparse ones' rows are inducing points */ };
// a copy made from the fit-type L^-1 in `linv`.  Deferred: made when something first asks for it
enum class Copy { Absent, Deferred, Valid };

struct Resident {
  // ---- the data
  bool have_data = false;   // x64 / y64 and their host mirrors hold the caller's rows AND targets
  bool have_s = false;      // sdiag / s_host hold a per-point noise vector for them
  bool sg_have = false;     // sgX / sgY hold the sparse models' training set
  bool sg_have_z = false;   // ... and the resident rows are its inducing points
  bool sg_factors = false;  // Kuf, Lu, LB, cv of the last gpso_sgpr_bound_u are still in their buffers (gpso_sgpr_get_factor)
  // ---- the posterior
  Post post = Post::None;
  bool has_post() const { return post != Post::None; }
  // no targets, no factor of its own: no append, no self-test (the sparse kinds' rows are Z, not the data)
  bool variational() const { return post == Post::Vgp || post == Post::Sgpr || post == Post::Svgp; }
  // ---- copies derived from it
  bool chol_valid = false;     // Lf / linv hold the factor and its inverse in the fit type
  bool have_kinv = false;      // kinvb holds K^-1 (a fit that returned a gradient)
  Copy linv_p = Copy::Absent;  // the packed f32 / f64 L^-1 of the native tile kernel (a receiver of a split posterior: absent)
  Copy linv_b = Copy::Absent;  // the 16-bit split pieces (deferred by a fit that returned a gradient: ensure_split_pieces)
  int small_tile_rows = 8;     // tile rows of the 128-padded linv_p that may be non-zero (8: all / unknown)
  bool paths_valid = false;    // the path set of gpso_paths_draw / gpso_paths_draw_q (omega, b, w, v) belongs to this posterior as it stands
  bool q_factors = false;      // a variational install's Lu (Lf), beta (alpha_f) and root Q of q (vq_S / svq_S / sgM2) are still in their buffers
  bool bernoulli = false;      // a Post::Vgp install under GPSO_LIK_BERNOULLI: (mean, var) are the latent's, noise slot 0 (success.hpp)
  bool screen_refused = false;  // a screened best-UCB call on this posterior was refused (a flat mean prunes nothing): it is not screened again
  // ---- the hyper-parameter ensemble (ensemble.hpp): its members are posteriors of the resident DATA at other theta, so a
  // refit leaves them alone and whatever changes the data, its noise vector or whose rows these are ends them: data_changed()
  bool ensemble = false;
  // ---- the constraint set (constraints.hpp): posteriors of OTHER targets, copied in from wherever they were fitted.  It
  // belongs to the context, not to the resident data: new data, a refit, an append and an install leave it alone (a scoring
  // call compares shapes); gpso_constraint_clear and gpso_alloc_posterior end it
  bool constraints = false;
  // ---- the success member (success.hpp): ONE Bernoulli-installed classifier posterior, copied in beside the constraint set
  // and with its lifetime: gpso_success_clear and gpso_alloc_posterior end it
  bool success = false;
  // ---- what the precision self-test ruled on it
  bool st_have = false;          // a posterior with targets is resident (one fitted here): the self-test can run
  bool st_done = false;          // st_vals are this posterior's, in the arithmetic now in use
  bool gen_eff32 = true;         // the cross-Gram tile is generated in float (GPSO_GEN_AUTO: until the self-test objects)
  bool gen_decided = false;      // AUTO: has the self-test ruled on this posterior?
  bool gen32_inputs_ok = false;  // xs32 / xnorm32 / xs_p32 match the resident posterior
  bool c16_fallback = false;     // this posterior's float generation keeps the f32 contraction (decide_generation)
  int math = GPSO_MATH_NATIVE;   // predict math: the caller's fixed choice, or the rung of GPSO_MATH_AUTO's ladder it stands on
  bool math_native_fallback = false;  // ... and the self-test preferred the f32 MFMA kernel for it
  // ---- what the peers of a group hold of it (gpso_broadcast_posterior_rows)
  int64_t sync_n = -1;      // rows the peers hold; -1: unknown
  int sync_math = -1;       // predict math in use then (the ladder may move: other pieces)
  float sync_scale = 0.0f;  // fp16 split: the scale the peers' planes were packed with

  explicit Resident(int first_math) : math(first_math) {}
  bool split_usable(bool float_predict, int64_t npad) const {
    return float_predict && math != GPSO_MATH_NATIVE && !math_native_fallback && npad > 0 && npad % 256 == 0;
  }

  // ==== transitions ====
  // What every call that replaces the posterior shares.  linv_b stays as it was found: every way to a new factor packs,
  // defers or drops the pieces again.
  // keep_peers: gpso_sgpr_select_inducing alone -- where it fails (a rank-deficient Gram) the peers record survives, and a
  // gpso_adopt_posterior with no gpso_alloc_posterior before it would still meet it in gpso_broadcast_posterior_rows
  void posterior_dropped(bool keep_peers = false) {
    post = Post::None;
    have_kinv = chol_valid = st_done = st_have = false;
    linv_p = Copy::Absent;
    paths_valid = q_factors = screen_refused = bernoulli = false;
    if (!keep_peers) sync_n = -1;
  }
  void success_pushed() { success = true; }    // gpso_success_push succeeded
  void success_cleared() { success = false; }  // gpso_success_clear
  void constraint_pushed() { constraints = true; }      // gpso_constraint_push succeeded
  void constraints_cleared() { constraints = false; }  // gpso_constraint_clear
  void ensemble_pushed() { ensemble = true; }     // gpso_ensemble_push succeeded
  void ensemble_cleared() { ensemble = false; }  // gpso_ensemble_clear
  // the rows, their targets or their noise are no longer what the ensemble's members were fitted on
  void data_changed() { ensemble = false; }
  void screen_was_refused() { screen_refused = true; }  // posterior_dropped() and appended() end it
  // A new posterior begins (or an option changed): generation starts over -- float unless double was asked for --, the
  // ladder on its first rung, and the self-test rules again.  Not part of posterior_dropped(): new data, a new noise
  // vector, moved inducing rows and a hand-off's allocation keep the old verdicts until the next posterior begins
  void reset_generation(bool float_predict, bool math_auto, int gen_mode) {
    math_native_fallback = false;
    if (math_auto) math = float_predict ? GPSO_MATH_F16X3 : GPSO_MATH_NATIVE;
    gen_eff32 = float_predict && gen_mode != GPSO_GEN_F64;
    gen_decided = gen32_inputs_ok = c16_fallback = st_done = false;
  }
  // -- the data.  as_inducing: the rows are the Z that gpso_sgpr_set_inducing puts beside the stashed training set
  void new_data(bool as_inducing) {
    have_data = true;
    data_changed();
    have_s = sg_factors = false;  // (the per-point noise belonged to the rows just replaced)
    sg_have_z = as_inducing;
    if (!as_inducing) sg_have = false;
    posterior_dropped();
  }
  void noise_changed(bool have_vector) { have_s = have_vector; sg_factors = false; data_changed(); posterior_dropped(); }
  void stashed() { sg_have = true; sg_have_z = false; }
  void rows_unknown() { sg_have = sg_have_z = have_data = false; data_changed(); }  // an upload of Z failed half-way
  void inducing_moved() { sg_factors = false; data_changed(); posterior_dropped(); }  // same M, in place: the data and q stay
  void selection_begun() { sg_factors = false; data_changed(); posterior_dropped(true); }
  void bound_ready() { sg_factors = true; }  // gpso_sgpr_bound_u succeeded
  // -- the exact GP (each *_begun is followed by reset_generation)
  // rows: the tile rows of linv_p this fit writes (a one-launch fit's own; else 8) -> those that may hold older data
  int fit_begun(int rows) {
    sg_have_z = sg_factors = false;  // (the rows are no inducing points any more)
    posterior_dropped();
    return std::exchange(small_tile_rows, rows);
  }
  // split_deferred: beside a gradient the pieces wait for the first predict-type call (else pack_bf16 has ruled)
  void fit_done(bool grad, bool linv_p_deferred, bool split_deferred, bool split_usable_now) {
    post = Post::Fitted;
    chol_valid = st_have = true;
    have_kinv = grad;
    linv_p = linv_p_deferred ? Copy::Deferred : Copy::Valid;
    if (split_deferred) linv_b = split_usable_now ? Copy::Deferred : Copy::Absent;
  }
  void paths_drawn() { paths_valid = true; }  // gpso_paths_draw(_q) succeeded; posterior_dropped() and appended() end it
  void split_packed(bool built) { linv_b = built ? Copy::Valid : Copy::Absent; }  // pack_bf16 began / ended
  void linv_p_packed() { small_tile_rows = 8; linv_p = Copy::Valid; }
  // the self-test looks at the extended posterior; the float copies of the inputs are derived again
  void appended(bool first_noise_vector) {
    have_s = have_s || first_noise_vector;
    data_changed();
    have_kinv = st_done = gen32_inputs_ok = paths_valid = screen_refused = false;  // (v was solved against the shorter factor)
    small_tile_rows = 8;
  }
  void append_refused() { gen32_inputs_ok = false; }  // not PD: the scaled inputs were put back, their float copies not
  void install_begun() {  // y unknown: a later fit needs gpso_set_data (and gpso_set_noise_diag behind it)
    have_data = have_s = sg_have = sg_have_z = sg_factors = false;
    data_changed();
    small_tile_rows = 8;  // (linv_p is about to be written whole)
    posterior_dropped();
  }
  void installed() { post = Post::Installed; chol_valid = true; linv_p = Copy::Valid; }
  // -- the variational families (reset_generation follows).  A VGP call leaves sg_factors alone, the sparse ones drop it
  void variational_begun(bool sparse) { if (sparse) sg_factors = false; data_changed(); posterior_dropped(); }
  // linv_p was written whole either way; ok: linv holds C = R L^-1 and every factorisation succeeded.  The install's own
  // factors stay where gpso_paths_draw_q reads them until variational_begun() -- every call that writes Lf, q or the sparse
  // factors starts with it -- or any other drop of the posterior: q_factors_kept() / posterior_dropped()
  void variational_ready(Post kind, bool ok) {
    small_tile_rows = 8;
    if (ok) { post = kind; chol_valid = true; linv_p = Copy::Valid; q_factors_kept(); }
  }
  // (at present implied by a variational kind with chol_valid: nothing clears it alone)
  void q_factors_kept() { q_factors = true; }
  void bernoulli_installed() { bernoulli = true; }  // gpso_vgp_posterior under the Bernoulli kind succeeded; posterior_dropped() ends it
  // -- hand-off
  void recarved() { small_tile_rows = 8; linv_b = linv_p = Copy::Absent; }  // the arena's slices moved: another layout's bytes
  // gpso_alloc_posterior: as for gpso_set_posterior, the rows about to arrive are neither data nor inducing points of this
  // context.  have_s stays: the variational entry points refuse on it with GPSO_E_ARG before they look for data
  void shape_allocated() { have_data = sg_have = sg_have_z = sg_factors = false; data_changed(); constraints_cleared(); success_cleared(); posterior_dropped(); }
  // slot 7 of the hyper block, which travels: 1 = float generation, 2 = GPSO_MATH_AUTO settled on the f32 MFMA kernel,
  // 4 = the split pieces are built, 8 = the packed L^-1 travels too, 16 = float generation keeps the f32 contraction,
  // 256 x the predict math (which split the pieces are: a receiver under GPSO_MATH_AUTO follows)
  double handoff_word(bool gen_double, bool split_usable_now, bool with_linv_p) const {
    return (gen_double ? 0.0 : 1.0) + (math_native_fallback ? 2.0 : 0.0) + ((split_usable_now && linv_b == Copy::Valid) ? 4.0 : 0.0) +
           ((with_linv_p && linv_p == Copy::Valid) ? 8.0 : 0.0) + (c16_fallback ? 16.0 : 0.0) + 256.0 * math;
  }
  // generation arithmetic and predict math: the sender's choice (its self-test ruled), unless this context insists
  void adopted(int sender, bool float_predict, bool math_auto, int gen_mode, int64_t npad) {
    post = Post::Adopted;
    data_changed();
    chol_valid = have_kinv = paths_valid = q_factors = screen_refused = false;
    small_tile_rows = 8;         // linv_p came from elsewhere
    st_done = st_have = false;   // the fitting rank ran the self-test; no targets here
    math_native_fallback = math_auto && (sender & 2) != 0;
    const int sender_math = sender >> 8;
    if (math_auto && float_predict && (sender_math == GPSO_MATH_F16X3 || sender_math == GPSO_MATH_BF16X6)) math = sender_math;
    // the split pieces the sender actually built travel with it (and are the split this context runs)
    linv_b = (split_usable(float_predict, npad) && (sender & 4) != 0 && sender_math == math) ? Copy::Valid : Copy::Absent;
    linv_p = (sender & 8) != 0 ? Copy::Valid : Copy::Absent;
    gen_eff32 = float_predict && (gen_mode == GPSO_GEN_F32 || (gen_mode == GPSO_GEN_AUTO && (sender & 1) != 0));
    gen_decided = true;
    gen32_inputs_ok = false;
    c16_fallback = (sender & 16) != 0;  // (the sender's float generation kept the f32 contraction: same arithmetic here)
  }
  void peers_hold(int64_t n, int math_in_use, float scale) { sync_n = n; sync_math = math_in_use; sync_scale = scale; }
  // gpso_broadcast_posterior on a receiver under GPSO_MATH_AUTO: the root's rung, or the f32 MFMA kernel
  void ladder_follows(int root_math, bool float_predict) {
    math_native_fallback = root_math == GPSO_MATH_NATIVE && float_predict;
    if (root_math != GPSO_MATH_NATIVE) math = root_math;
  }
  // -- options
  void math_chosen(int value) { math = value; linv_b = Copy::Absent; }  // (reset_generation follows)
  void contraction_changed() { gen_decided = st_done = false; }         // (other bits: the self-test rules again)
  // -- the self-test's rulings
  void selftest_ran() { st_done = true; }
  void gen_inputs_made() { gen32_inputs_ok = true; }
  // decide_generation: an arithmetic to measure next; then the ruling (with arguments: st_vals hold ITS readings already)
  void generation_trial(bool float32, bool f32_contraction) { gen_eff32 = float32; c16_fallback = f32_contraction; st_done = false; }
  void generation_ruled() { gen_decided = true; }
  void generation_ruled(bool float32, bool f32_contraction) { gen_eff32 = float32; c16_fallback = f32_contraction; gen_decided = true; }
  // GPSO_MATH_AUTO, the self-test failed on this rung: the next split, or (GPSO_MATH_NATIVE) the f32 MFMA kernel
  void ladder_down(int rung) {
    if (rung == GPSO_MATH_NATIVE) math_native_fallback = true;
    else math = rung;
    st_done = false;
  }
};

}  // namespace gpso
