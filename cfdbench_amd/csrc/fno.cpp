// Whole Auto-FNO forward / backward as one C call each (Fno2d.forward, src/models/fno/fno2d.py:178-242, and the
// autograd pass behind loss["nmse"].backward(), src/train_auto.py:255).  Only enqueues kernels on `stream`.
//
// Activation storage: block l keeps its PRE-activation a_{l+1} = spectral(h_l) + w0 h_l + b (h_0 = a_0 = fc0 output,
// h_l = gelu(a_l) for l >= 1); consumers apply GELU on load (act_in=1) so every activation crosses HBM once per
// producer/consumer instead of once more for a standalone GELU pass, and the backward pass reads the same buffers.
#include "cfd_common.h"
#include "cfd_tail.h"

namespace {

struct Layout {
    size_t n_act;    // floats of one (B,C,H,W) activation
    size_t n_modes;  // floats of one (B,C,2*m1,m2) complex tensor
    size_t off_acts, off_xh, off_z, off_gA, off_gB, off_gh, off_scratch, off_tmp;
    size_t off_crop, off_coord;  // pad > 0 only: a_L cropped to the data grid (B,C,H,W) fp32; the data grid's coordinate tables
    size_t n_crop;               // floats of one (B,C,H,W) activation on the data grid
    // byte offsets inside the scratch region (training only): the 1x1 weight-gradient partials, the lifting layer's sum records, the
    // training head's partial records
    size_t off_chan_part, off_stemg, head_off;
    size_t scratch_bytes, total_bytes;
    int n_acts, n_xh;
};

size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// The host-side view of `p` the lifting layer's gradient takes on a padded shape: the DATA grid's extents and coordinate tables (`coords`:
// the table k_stem_pad left in the workspace).  Only H, W, d_gx and d_gy of a plan are read on that path.  pad == 0: the plan itself.
cfd_plan data_plan(const cfd_plan* p, const cfd_fno_shape* s, float* coords) {
    cfd_plan dp = *p;
    if (s->pad > 0) {
        dp.H = s->H;
        dp.W = s->W;
        dp.d_gx = coords;
        dp.d_gy = coords ? coords + CFD_PAD_COORD_GY : nullptr;
    }
    return dp;
}

Layout make_layout(const cfd_plan* p, const cfd_fno_shape* s, int training, int dt = CFD_DT_F32) {
    Layout L{};
    const size_t esz = cfd_dt_size(dt);  // bytes of one stored activation
    // domain padding (shape.pad > 0): activations, input gradients and everything a block phase sizes live on the padded grid HWp (the
    // plan's); the head, the loss and the lifting layer's gradient on the data grid HW.  pad == 0: HWp == HW, the layout of every earlier ABI.
    const size_t HW = (size_t)s->H * s->W, HWp = (size_t)(s->H + s->pad) * (s->W + s->pad);
    const int C = s->hidden, B = s->B;
    L.n_act = (size_t)B * C * HWp;
    L.n_crop = (size_t)B * C * HW;
    L.n_modes = (size_t)B * C * 2 * s->modes1 * s->modes2 * 2;
    L.n_acts = training ? s->num_layers + 1 : 2;
    L.n_xh = training ? s->num_layers : 1;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += cfd_align_up(bytes, 256); return o; };
    L.off_acts = take(L.n_act * esz * L.n_acts);
    L.off_xh = take(L.n_modes * sizeof(float) * L.n_xh);
    L.off_z = take(L.n_modes * sizeof(float));
    L.off_tmp = dt == CFD_DT_BF16 ? take(L.n_act * sizeof(float)) : 0;  // fp32 result of the 1x1 conv (bf16 storage path)
    size_t scratch = cfd_fno_head_workspace_bytes(B, C, s->head, s->out_chan, (int)HW);
    if (training) {
        L.off_gA = take(L.n_act * sizeof(float));
        L.off_gB = take(L.n_act * sizeof(float));
        L.off_gh = take(L.n_modes * sizeof(float));
        // both weight-gradient partial buffers of a block are alive until the block's input-gradient kernel has reduced
        // them (cfd_tail.h): spectral partials first, the 1x1-conv partials behind them
        L.off_chan_part = cfd_align_up(cfd_spectral_wgrad_workspace_bytes(p, B, C, C), 256);
        const size_t block_part = L.off_chan_part + cfd_chan_wgrad_workspace_bytes(B, C, C, (int)HWp);
        scratch = max2(scratch, block_part);
        const cfd_plan dp = data_plan(p, s, nullptr);
        scratch = max2(scratch, cfd_fno_stem_bwd_workspace_bytes(&dp, B, s->in_chan, s->n_case_params, C));
        // the lifting layer's sums of k_block<.., STEMG> live behind the two weight-gradient partial regions of the last block phase (which
        // the tail workgroups of the same launch are still reading)
        L.off_stemg = cfd_align_up(block_part, 256);
        scratch = max2(scratch, L.off_stemg + cfd_int_stemg_part_bytes(p, B, C));
        // round 6: the training head's partial records behind everything a block phase writes -- with CFD_TRAIN_DEFER_HEAD they are read
        // by backward phase 1's block kernel, AFTER that phase's weight-gradient producers have written their partials into the regions above
        L.head_off = cfd_align_up(L.off_stemg + cfd_int_stemg_part_bytes(p, B, C), 256);
        scratch = max2(scratch, L.head_off + cfd_fno_head_workspace_bytes(B, C, s->head, s->out_chan, (int)HW));
    }
    L.scratch_bytes = scratch;
    L.off_scratch = take(scratch);
    if (s->pad > 0) {
        L.off_crop = take(L.n_crop * sizeof(float));
        L.off_coord = take(CFD_PAD_COORD_FLOATS * sizeof(float));
    }
    L.total_bytes = off;
    return L;
}

// hidden 33 .. CFD_WIDE_MAX: the wide-channel route (wide.hip), fp32 activation storage only; the same for many-modes plans (dft_many.hip)
int check_shape(const char* fn, const cfd_plan* p, const cfd_fno_shape* s, int dt = CFD_DT_F32) {
    CFD_REQUIRE(p && s, CFD_ERR_INVALID_ARG, "%s: NULL plan/shape", fn);
    CFD_REQUIRE(s->pad >= 0, CFD_ERR_INVALID_ARG, "%s: pad=%d (0 = no domain padding)", fn, s->pad);
    CFD_REQUIRE(s->pad == 0 || (s->H >= 2 && s->W >= 2), CFD_ERR_INVALID_ARG, "%s: pad=%d needs a data grid of at least 2x2 (got %dx%d)", fn,
                s->pad, s->H, s->W);
    // the plan is the grid the FnoBlocks run on: the data grid plus `pad` rows at the bottom and `pad` columns at the right
    CFD_REQUIRE(p->H == s->H + s->pad && p->W == s->W + s->pad && p->m1 == s->modes1 && p->m2 == s->modes2, CFD_ERR_INVALID_ARG,
                "%s: plan is for %dx%d modes (%d,%d) but shape says data grid %dx%d + pad %d = %dx%d modes (%d,%d)", fn, p->H, p->W, p->m1,
                p->m2, s->H, s->W, s->pad, s->H + s->pad, s->W + s->pad, s->modes1, s->modes2);
    CFD_REQUIRE(s->pad == 0 || dt == CFD_DT_F32, CFD_ERR_UNSUPPORTED, "%s: pad=%d: bf16 activation storage needs pad = 0", fn, s->pad);
    CFD_REQUIRE(s->B >= 1, CFD_ERR_INVALID_ARG, "%s: empty batch", fn);
    CFD_REQUIRE(s->num_layers >= 0 && s->num_layers <= CFD_MAX_LAYERS, CFD_ERR_UNSUPPORTED, "%s: num_layers=%d (max %d)", fn,
                s->num_layers, CFD_MAX_LAYERS);
    CFD_REQUIRE(s->hidden >= 1 && s->hidden <= CFD_WIDE_MAX, CFD_ERR_UNSUPPORTED, "%s: hidden=%d (max %d)", fn, s->hidden, CFD_WIDE_MAX);
    CFD_REQUIRE(s->hidden <= 32 || dt == CFD_DT_F32, CFD_ERR_UNSUPPORTED, "%s: hidden=%d: bf16 activation storage needs hidden <= 32", fn,
                s->hidden);
    CFD_REQUIRE(s->out_chan >= 1 && s->out_chan <= 8, CFD_ERR_UNSUPPORTED, "%s: out_chan=%d (max 8) unsupported", fn, s->out_chan);
    CFD_REQUIRE(s->out_chan <= 2 || dt == CFD_DT_F32, CFD_ERR_UNSUPPORTED, "%s: out_chan=%d: bf16 activation storage needs out_chan <= 2", fn,
                s->out_chan);
    CFD_REQUIRE(!p->many || dt == CFD_DT_F32, CFD_ERR_UNSUPPORTED,
                "%s: grid %dx%d, modes (%d,%d): bf16 activation storage needs modes1 <= 15, modes2 <= 16 and W <= 80", fn, p->H, p->W, p->m1,
                p->m2);
    // (only the general-width transforms read and write 2-byte activations, and their tables exist up to 70 rows: refused here, before
    // the lifting layer has written the workspace, not where the first transform would find no table)
    CFD_REQUIRE(dt == CFD_DT_F32 || (p->d_fwd_g && p->d_inv_g), CFD_ERR_UNSUPPORTED,
                "%s: grid %dx%d: bf16 activation storage needs H <= 70 and W <= 80", fn, p->H, p->W);
    // Grids wider than 80 columns: the pixel-domain kernels index activations with 32-bit products of at most B * max(hidden, head) * H * W
    // elements (at 128 x 128 and head width 128: B <= 1023): refuse what would wrap
    if (p->W > 80) {
        const long long widest = s->hidden > s->head ? s->hidden : s->head;
        CFD_REQUIRE((long long)s->B * widest * p->H * p->W <= 0x7fffffffLL, CFD_ERR_UNSUPPORTED,
                    "%s: B=%d at %dx%d, width %d: more than 2^31 - 1 activation elements per tensor", fn, s->B, p->H, p->W, (int)widest);
    }
    return CFD_OK;
}

// The workspace as one call sees it: the Layout and a view of every region.  Every entry builds one and does no offset arithmetic of its own.
struct View {
    Layout L;
    char* base;
    size_t act_stride;  // bytes of one stored activation
    bool training;
    View(const cfd_plan* p, const cfd_fno_shape* s, int training_, int dt, void* ws)
        : L(make_layout(p, s, training_, dt)), base((char*)ws), act_stride(L.n_act * cfd_dt_size(dt)), training(training_ != 0) {}
    // a_l: training keeps a_0 .. a_L for the backward pass, inference ping-pongs between two buffers
    void* act(int l) const { return base + L.off_acts + (size_t)(training ? l : (l & 1)) * act_stride; }
    float* xh(int l) const { return (float*)(base + L.off_xh) + (size_t)(training ? l : 0) * L.n_modes; }
    float* z() const { return (float*)(base + L.off_z); }
    float* tmp() const { return (float*)(base + L.off_tmp); }  // bf16 storage only
    float* gA() const { return (float*)(base + L.off_gA); }
    float* gB() const { return (float*)(base + L.off_gB); }
    float* gh() const { return (float*)(base + L.off_gh); }
    char* scratch() const { return base + L.off_scratch; }  // spectral weight-gradient partials (and whatever else is alone)
    char* scratch2() const { return scratch() + L.off_chan_part; }  // the 1x1 weight-gradient partials behind them
    float* stem_part() const { return (float*)(scratch() + L.off_stemg); }  // the lifting layer's sum records
    char* head_rec() const { return scratch() + L.head_off; }  // the training head's partial records
    float* crop() const { return (float*)(base + L.off_crop); }  // pad > 0 only
    float* coord() const { return (float*)(base + L.off_coord); }  // pad > 0 only
};

// THE route rule: which fusions and deferrals a call may use.  Evaluated once per entry; the forward call, every backward phase and
// cfd_fno_adam_step evaluate the same thing and so agree.  A shape is narrow unless one of the exclusions in the first column holds.
//
//                              stem_in_dft              stemg                    scale            head                       stem
//   hidden > 32                no (dft_stem_ok)         no (stemg_ok: C <= 24)   no               no                         no
//   p->many                    no (dft_stem_ok)         no (stemg_ok)            no               no                         no
//   out_chan > 2               as narrow                as narrow                no               no                         no
//   pad > 0                    no                       no                       no               no                         no
//   bf16 storage               no                       no                       as narrow        no                         no
//   num_layers == 0            no                       no                       as narrow        no                         no
//   grads->d_inputs or         as narrow                no                       no               no                         no
//     grads->d_case_params
//   narrow                     cfd_int_dft_stem_ok      cfd_int_stemg_ok         flag, which = 1  flag, block_bwd_fused      flag, stemg
//
// stem_in_dft: the lifting layer rides in the first forward transform (round 6: on 64 x 64 one launch and one activation-sized read less).
//   Not with domain padding: the fused kernel writes the unpadded layout with the plan's coordinates.
// stemg: round 5: where the fused FnoBlock kernel runs the last block phase (l = 0), it emits the six per-(entry, channel) sums the lifting
//   layer's gradient needs instead of storing g_0 for a pass that reads it back (cfd_tail.h: CfdStemG): one activation-sized write and the
//   k_chan_wgrad_stem launch less.  Not with domain padding: g_0 lives on the padded grid and the sums would be taken with the plan's coordinates.
// scale / head / stem: the CFD_TRAIN_DEFER_* bits of `flags` that apply.  The wide route, the many-modes route and the head's channel route
//   have none of the fused kernels that carry a deferred job, and a padded shape's lifting layer and head are kernels of their own (pad.hip):
//   every flag is ignored there.  scale is the only one that bf16 storage keeps; stem implies stemg.
// grads->d_inputs / d_case_params (ABI 603): the input gradients are taken from g_0 in memory (ingrad.hip), so the block kernel must store
//   it (no stemg, hence no stem), and they are final after the pass: a deferred normaliser would leave them short of its factor, and the
//   head's deferral goes with it so that the route is the unfused one as a whole.  The forward trunk is untouched.
struct Route {
    bool stem_in_dft, stemg;
    bool scale, head, stem;
};
bool wants_ingrad(const cfd_fno_params* g) { return g && (g->d_inputs || g->d_case_params); }
Route route(const cfd_plan* p, const cfd_fno_shape* s, const View& v, int which, int dt, int flags, const void* inputs, const void* mask,
            const cfd_fno_params* grads) {
    const int B = s->B, C = s->hidden, NL = s->num_layers;
    const bool fusable = s->pad == 0 && dt == CFD_DT_F32 && NL >= 1;
    const bool ingrad = wants_ingrad(grads);
    const bool defers = !(C > 32 || p->many || s->out_chan > 2 || s->pad > 0 || ingrad);
    Route r{};
    r.stem_in_dft = fusable && cfd_int_dft_stem_ok(p, B, s->in_chan, s->n_case_params, C, inputs, mask, v.act(0));
    if (!v.training) return r;  // (inference has no gradient and defers nothing)
    r.stemg = fusable && !ingrad && cfd_int_stemg_ok(p, B, C, s->in_chan, s->n_case_params, inputs, mask, v.z());
    r.scale = defers && (flags & CFD_TRAIN_DEFER_SCALE) && which == 1;
    // backward phase 1 = FnoBlock NL-1: gcur = gA, gnext = gB, aprev = a_{NL-1} when NL > 1
    r.head = defers && fusable && (flags & CFD_TRAIN_DEFER_HEAD) && cfd_int_block_bwd_fused(p, B, C, v.gA(), v.gB(), NL > 1 ? v.act(NL - 1) : nullptr, v.z());
    r.stem = defers && (flags & CFD_TRAIN_DEFER_STEM) && r.stemg;
    return r;
}

// The trunk: lifting layer and FnoBlocks, a_0 .. a_L into v.act() (Fno2d.forward up to fc1, fno2d.py:178-224)
int trunk(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm, const View& v, const Route& rt, int dt, const float* inputs,
          const float* case_params, const float* mask, void* stream) {
    const int B = s->B, C = s->hidden, HWp = p->H * p->W, NL = s->num_layers;
    if (s->pad > 0)  // the lifting layer on the data grid, written into the padded layout with its zero band (pad.hip)
        CFD_TRY(cfd_int_stem_pad(inputs, mask, case_params, prm->fc0_w, prm->fc0_b, (float*)v.act(0), v.coord(), B, s->in_chan,
                                 s->n_case_params, C, s->H, s->W, s->pad, stream));
    else if (!rt.stem_in_dft)
        CFD_TRY(cfd_int_fno_stem_fwd(p, inputs, mask, case_params, prm->fc0_w, prm->fc0_b, v.act(0), B, s->in_chan, s->n_case_params, C, dt,
                                     stream));
    for (int l = 0; l < NL; ++l) {  // FnoBlock.forward, fno2d.py:106-112
        const int act = l > 0;
        if (l == 0 && rt.stem_in_dft)
            CFD_TRY(cfd_int_spectral_dft_stem(p, inputs, mask, case_params, prm->fc0_w, prm->fc0_b, (float*)v.act(0), v.xh(0), B,
                                              s->n_case_params, C, stream));
        else
            CFD_TRY(cfd_int_spectral_dft(p, v.act(l), v.xh(l), B * C, act, dt, stream));
        CFD_TRY(cfd_spectral_mix(p, v.xh(l), prm->spec_w1[l], prm->spec_w2[l], v.z(), B, C, C, 0, stream));
        if (dt == CFD_DT_F32) {
            CFD_TRY(cfd_fno_block_fwd(p, (const float*)v.act(l), v.z(), prm->w0_w[l], prm->w0_b[l], (float*)v.act(l + 1), B, C, C, act, stream));
        } else {  // bf16 storage: 1x1 conv into an fp32 scratch tensor, inverse transform added to it, ONE rounding on the store
            CFD_TRY(cfd_int_chanmix(v.act(l), prm->w0_w[l], prm->w0_b[l], v.tmp(), B, C, C, HWp, act, 0, dt, stream));
            CFD_TRY(cfd_int_spectral_idft(p, v.z(), v.tmp(), nullptr, v.act(l + 1), B * C, 1, dt, stream));
        }
    }
    return CFD_OK;
}

// What the head reads: a_L, or with domain padding x[..., :-pad, :-pad] (fno2d.py:225-226) cropped into the compact region -- the head
// kernels index flat H W
int head_input(const cfd_fno_shape* s, const View& v, void* stream, const void** aL) {
    *aL = v.act(s->num_layers);
    if (s->pad == 0) return CFD_OK;
    CFD_TRY(cfd_int_pad_crop((const float*)*aL, v.crop(), (long)s->B * s->hidden, s->H, s->W, s->pad, stream));
    *aL = v.crop();
    return CFD_OK;
}

}  // namespace

extern "C" size_t cfd_fno_workspace_bytes(const cfd_plan* p, const cfd_fno_shape* s, int training) {
    return cfd_fno_workspace_bytes_ex(p, s, training, CFD_DT_F32);
}

extern "C" size_t cfd_fno_workspace_bytes_ex(const cfd_plan* p, const cfd_fno_shape* s, int training, int act_dtype) {
    if (!p || !s || s->B < 1 || s->pad < 0 || (act_dtype != CFD_DT_F32 && act_dtype != CFD_DT_BF16)) return 0;
    return make_layout(p, s, training, act_dtype).total_bytes;
}

extern "C" int cfd_fno_forward(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm, const float* inputs,
                               const float* case_params, const float* mask, const float* label, float* preds,
                               float* sums, void* ws, int training, void* stream) {
    return cfd_fno_forward_ex(p, s, prm, inputs, case_params, mask, label, preds, sums, ws, training, CFD_DT_F32, stream);
}

// bf16 activation storage (act_dtype = 1, inference only): the activations between kernels -- the lifting layer's output, every
// FnoBlock's pre-activation -- are rounded to bf16 when stored and widened when loaded; inputs, predictions, kept modes,
// weights and all arithmetic stay fp32.  Halves the activation traffic of a rollout step (3.3 -> 1.7 MB per frame).
extern "C" int cfd_fno_forward_ex(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm, const float* inputs,
                                  const float* case_params, const float* mask, const float* label, float* preds,
                                  float* sums, void* ws, int training, int act_dtype, void* stream) {
    CFD_TRY(check_shape("cfd_fno_forward", p, s, act_dtype));
    CFD_REQUIRE(prm && inputs && preds && ws, CFD_ERR_INVALID_ARG, "cfd_fno_forward: NULL pointer");
    CFD_REQUIRE(!label || sums, CFD_ERR_INVALID_ARG, "cfd_fno_forward: label given without sums");
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || act_dtype == CFD_DT_BF16, CFD_ERR_INVALID_ARG, "cfd_fno_forward: act_dtype %d (0 = fp32, 1 = bf16)", act_dtype);
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || !training, CFD_ERR_UNSUPPORTED, "cfd_fno_forward: bf16 activation storage is an inference path (training = 0)");
    const int dt = act_dtype;
    const View v(p, s, training, dt, ws);
    const Route rt = route(p, s, v, 0, dt, 0, inputs, mask, nullptr);  // (flags = 0: this call defers nothing; the trunk reads stem_in_dft)
    CFD_TRY(trunk(p, s, prm, v, rt, dt, inputs, case_params, mask, stream));
    const void* aL;
    CFD_TRY(head_input(s, v, stream, &aL));
    CFD_TRY(cfd_int_fno_head_fwd(aL, mask, label, prm->fc1_w, prm->fc1_b, prm->fc2_w, prm->fc2_b, preds, sums, v.scratch(), s->B, s->hidden,
                                 s->head, s->out_chan, s->H * s->W, s->num_layers > 0, dt, stream));
    return CFD_OK;
}

// Training forward with the loss known in advance (FnoTrainEngine): everything of cfd_fno_forward(training = 1), but the
// projection head runs ONCE for both directions -- predictions, loss sums, d loss / d a_L and the head's parameter
// gradients leave the same kernel (head.hip, FUSE), so backward phase 0 is already done when this returns and the caller
// continues with cfd_fno_backward_phase(1 .. L+1).  `which` = 0 mse, 1 nmse, 2 mae; `upstream` = d objective / d loss.
extern "C" int cfd_fno_forward_train(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                     const cfd_fno_params* g, const float* inputs, const float* case_params,
                                     const float* mask, const float* label, float* preds, float* sums, float* coef, void* ws,
                                     int which, float upstream, void* stream) {
    return cfd_fno_forward_train_ex(p, s, prm, g, inputs, case_params, mask, label, preds, sums, coef, ws, which, upstream, CFD_DT_F32, stream);
}

// act_dtype = 1: bf16-storage TRAINING (the fork's other trainers offer mixed precision, src/args.py:77-80): the saved
// activations a_0 .. a_L are rounded to bf16 when stored (half the bytes of everything the backward pass re-reads); parameters,
// kept modes, gradients, accumulation and the optimiser stay fp32.  The backward pass differentiates the computation that was
// actually run, i.e. it reads the ROUNDED activations (cfd_fno_backward_phase_ex with the same act_dtype).  Each FnoBlock runs as
// 1x1 conv (fp32 scratch) + inverse transform with addend, so a stored pre-activation is rounded exactly once.
extern "C" int cfd_fno_forward_train_ex(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                        const cfd_fno_params* g, const float* inputs, const float* case_params,
                                        const float* mask, const float* label, float* preds, float* sums, float* coef, void* ws,
                                        int which, float upstream, int act_dtype, void* stream) {
    return cfd_fno_forward_train_f(p, s, prm, g, inputs, case_params, mask, label, preds, sums, coef, ws, which, upstream, act_dtype, 0, stream);
}

// flags: CFD_TRAIN_DEFER_* (include/cfdbench_amd.h) -- the single-GPU training step with its three tiny launches folded into others
extern "C" int cfd_fno_forward_train_f(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                       const cfd_fno_params* g, const float* inputs, const float* case_params,
                                       const float* mask, const float* label, float* preds, float* sums, float* coef, void* ws,
                                       int which, float upstream, int act_dtype, int flags, void* stream) {
    CFD_TRY(check_shape("cfd_fno_forward_train", p, s, act_dtype));
    CFD_REQUIRE(which >= 0 && which <= 2, CFD_ERR_INVALID_ARG, "cfd_fno_forward_train: which must be 0 (mse), 1 (nmse), 2 (mae)");
    CFD_REQUIRE(prm && g && inputs && label && preds && sums && ws && (coef || ((flags & CFD_TRAIN_DEFER_SCALE) && which == 1)), CFD_ERR_INVALID_ARG,
                "cfd_fno_forward_train: NULL pointer");
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || act_dtype == CFD_DT_BF16, CFD_ERR_INVALID_ARG, "cfd_fno_forward_train: act_dtype %d (0 = fp32, 1 = bf16)", act_dtype);
    const int dt = act_dtype;
    const View v(p, s, 1, dt, ws);
    CFD_REQUIRE(dt == CFD_DT_F32 || !wants_ingrad(g), CFD_ERR_UNSUPPORTED,
                "cfd_fno_forward_train: grads->d_inputs / d_case_params need fp32 activation storage");
    const Route rt = route(p, s, v, which, dt, flags, inputs, mask, g);
    const int B = s->B, C = s->hidden, HW = s->H * s->W, NL = s->num_layers, pad = s->pad;  // HW: the data grid
    // the label's energy and the gradient coefficients: independent of the network (scratch is free until the head); with
    // side_stream bit 1 they run beside the lifting layer on the side stream and join in front of the head (off by default:
    // the fork / join pair costs more than the 16 us it hides -- side.cpp)
    hipStream_t side = cfd_side_fork((hipStream_t)stream, rt.scale ? 0 : 1);
    if (!rt.scale) CFD_TRY(cfd_label_energy_coef(label, mask, sums, coef, v.scratch(), B, s->out_chan, HW, which, upstream, side));
    CFD_TRY(trunk(p, s, prm, v, rt, dt, inputs, case_params, mask, stream));
    CFD_TRY(cfd_side_join((hipStream_t)stream, side));
    // Domain padding: the head runs on the data grid -- a_L cropped into the compact region, d loss / d a_L written compactly into gB
    // (free until backward phase 1 writes it) and embedded into gA with a zero band: what autograd's slice backward produces.
    const void* aL;
    CFD_TRY(head_input(s, v, stream, &aL));
    float* ga = pad > 0 ? v.gB() : v.gA();
    if (C > 32) {  // wide route: the two passes behind cfd_int_fno_head_train (sums[2..3] and coef came from cfd_label_energy_coef)
        CFD_TRY(cfd_int_fno_head_train(aL, mask, label, coef, prm->fc1_w, prm->fc1_b, prm->fc2_w, prm->fc2_b, preds, sums, ga, g->fc1_w, g->fc1_b,
                                       g->fc2_w, g->fc2_b, v.scratch(), B, C, s->head, s->out_chan, HW, NL > 0, dt, stream));
    } else {
        // deferred normaliser: the mse coefficient by value, sum (label*mask)^2 and the count leave the head's reduction (sums[2], sums[3])
        const float count = (float)((double)B * s->out_chan * HW);
        HeadTail ht{};
        CFD_TRY(cfd_int_fno_head_train_f(aL, mask, label, rt.scale ? nullptr : coef, upstream / count, 0.f, rt.scale ? count : 0.f,
                                         prm->fc1_w, prm->fc1_b, prm->fc2_w, prm->fc2_b, preds, sums, ga, g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b,
                                         v.head_rec(), B, C, s->head, s->out_chan, HW, NL > 0, dt, stream, rt.head ? &ht : nullptr));
    }
    if (pad > 0) CFD_TRY(cfd_int_pad_embed(ga, v.gA(), (long)B * C, s->H, s->W, pad, stream));
    return CFD_OK;
}

// One phase of the backward pass: 0 = projection head (+ loss gradient), 1 .. L = FnoBlock L-phase (the blocks in reverse
// order), L+1 = lifting layer.  Phases must run in this order on one stream; the running input gradient alternates
// between two workspace buffers, so a phase finds its operands from its index alone.  After phase k the gradients of
// that phase's parameters are final -- a data-parallel trainer can start their all-reduce while later phases compute.
extern "C" int cfd_fno_backward_phase(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                      const cfd_fno_params* g, const float* inputs, const float* case_params,
                                      const float* mask, const float* label, const float* preds,
                                      const float* gpreds_ext, const float* coef, void* ws, int phase, void* stream) {
    return cfd_fno_backward_phase_ex(p, s, prm, g, inputs, case_params, mask, label, preds, gpreds_ext, coef, ws, phase, CFD_DT_F32, stream);
}

// act_dtype = 1 continues cfd_fno_forward_train_ex(act_dtype = 1): phases 1 .. L+1 read the bf16 activations that pass stored.  (Phase 0,
// the stand-alone head backward, exists for fp32 storage only: the bf16 path always runs the one-pass training head.)
extern "C" int cfd_fno_backward_phase_ex(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                         const cfd_fno_params* g, const float* inputs, const float* case_params,
                                         const float* mask, const float* label, const float* preds,
                                         const float* gpreds_ext, const float* coef, void* ws, int phase, int act_dtype, void* stream) {
    return cfd_fno_backward_phase_f(p, s, prm, g, inputs, case_params, mask, label, preds, gpreds_ext, coef, nullptr, ws, phase, 0, act_dtype, 0, stream);
}

// flags (CFD_TRAIN_DEFER_*): phase 1 carries the head's reduction left behind by cfd_fno_forward_train_f (which needs `sums` and `which`
// again: the head job writes the loss sums); phase L + 1 launches nothing when cfd_fno_adam_step finishes the lifting layer's gradient.
extern "C" int cfd_fno_backward_phase_f(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                        const cfd_fno_params* g, const float* inputs, const float* case_params,
                                        const float* mask, const float* label, const float* preds,
                                        const float* gpreds_ext, const float* coef, float* sums, void* ws, int phase, int which,
                                        int act_dtype, int flags, void* stream) {
    CFD_TRY(check_shape("cfd_fno_backward_phase", p, s, act_dtype));
    CFD_REQUIRE(prm && g && inputs && ws, CFD_ERR_INVALID_ARG, "cfd_fno_backward_phase: NULL pointer");
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || act_dtype == CFD_DT_BF16, CFD_ERR_INVALID_ARG, "cfd_fno_backward_phase: act_dtype %d (0 = fp32, 1 = bf16)", act_dtype);
    const int dt = act_dtype;
    CFD_REQUIRE(dt == CFD_DT_F32 || !wants_ingrad(g), CFD_ERR_UNSUPPORTED,
                "cfd_fno_backward_phase: grads->d_inputs / d_case_params need fp32 activation storage");
    const View v(p, s, 1, dt, ws);
    const int B = s->B, C = s->hidden, HW = s->H * s->W, HWp = p->H * p->W, NL = s->num_layers, pad = s->pad;  // HW: data grid, HWp: the plan's
    CFD_REQUIRE(phase >= 0 && phase <= NL + 1, CFD_ERR_INVALID_ARG, "cfd_fno_backward_phase: phase %d outside 0..%d", phase, NL + 1);
    if (phase == 0) {
        CFD_REQUIRE(dt == CFD_DT_F32, CFD_ERR_UNSUPPORTED, "cfd_fno_backward_phase: phase 0 with bf16 storage (the head ran in cfd_fno_forward_train_ex)");
        // Domain padding: the head on the data grid -- a_L as the forward call cropped it, the gradient compact in gB, embedded into gA
        const float* aL = pad > 0 ? v.crop() : (const float*)v.act(NL);
        float* ga = pad > 0 ? v.gB() : v.gA();
        CFD_TRY(cfd_fno_head_bwd(aL, mask, label, preds, gpreds_ext, coef, prm->fc1_w, prm->fc1_b, prm->fc2_w, ga, g->fc1_w, g->fc1_b, g->fc2_w,
                                 g->fc2_b, v.scratch(), B, C, s->head, s->out_chan, HW, NL > 0, stream));
        return pad > 0 ? cfd_int_pad_embed(ga, v.gA(), (long)B * C, s->H, s->W, pad, stream) : CFD_OK;
    }
    const int done = phase - 1;  // blocks already processed: the gradient sits in gA after an even count
    float* gcur = (done & 1) ? v.gB() : v.gA();
    float* gnext = (done & 1) ? v.gA() : v.gB();
    const Route rt = route(p, s, v, which, dt, flags, inputs, mask, g);
    CFD_REQUIRE(!rt.head || sums, CFD_ERR_INVALID_ARG, "cfd_fno_backward_phase: CFD_TRAIN_DEFER_HEAD needs the `sums` of the forward call");
    if (phase == NL + 1) {
        if (rt.stem) return CFD_OK;  // cfd_fno_adam_step's launch finishes the lifting layer's gradient
        if (rt.stemg) return cfd_int_stemg_combine(p, v.stem_part(), case_params, g->fc0_w, g->fc0_b, B, C, s->in_chan, s->n_case_params, stream);
        // Domain padding: g_0 cropped into the free gradient buffer; the lifting layer's gradient on the data grid with ITS coordinates
        const float* g0 = gcur;
        if (pad > 0) {
            CFD_TRY(cfd_int_pad_crop(gcur, gnext, (long)B * C, s->H, s->W, pad, stream));
            g0 = gnext;
        }
        const cfd_plan dp = data_plan(p, s, v.coord());
        CFD_TRY(cfd_fno_stem_bwd(&dp, g0, inputs, mask, case_params, g->fc0_w, g->fc0_b, v.scratch(), B, s->in_chan, s->n_case_params, C, stream));
        if (!wants_ingrad(g)) return CFD_OK;
        // d loss / d inputs, d loss / d case_params from the same g_0 (the cropped one with domain padding); its partial records go where the
        // lifting layer's weight gradient has just finished with its own (same stream), so the workspace does not grow
        return cfd_int_fno_ingrad(g0, prm->fc0_w, g->d_inputs, g->d_case_params, v.scratch(),
                                  cfd_fno_stem_bwd_workspace_bytes(&dp, B, s->in_chan, s->n_case_params, C), B, s->in_chan, s->n_case_params, C,
                                  HW, stream);
    }
    const int l = NL - phase;
    const int act = l > 0;
    // gcur = d loss / d a_{l+1}
    if (dt == CFD_DT_BF16) {
        // two passes for the input gradient (1x1 conv transposed into the fp32 scratch tensor, inverse transform + addend
        // [* gelu'(a_l), a_l read as bf16]); the weight-gradient producers reduce their own partial sums
        CFD_TRY(cfd_spectral_dft(p, gcur, v.gh(), B * C, 0, stream));
        CFD_TRY(cfd_int_spectral_mix_adj_wgrad(p, v.xh(l), v.gh(), prm->spec_w1[l], prm->spec_w2[l], v.z(), g->spec_w1[l], g->spec_w2[l],
                                               v.scratch(), B, C, C, stream, nullptr));
        CFD_TRY(cfd_int_chan_wgrad_dt(gcur, v.act(l), g->w0_w[l], g->w0_b[l], v.scratch2(), B, C, C, HWp, act, dt, stream, nullptr));
        CFD_TRY(cfd_chanmix(gcur, prm->w0_w[l], nullptr, v.tmp(), B, C, C, HWp, 0, 1, stream));
        return cfd_int_spectral_idft_grad(p, v.z(), v.tmp(), act ? v.act(l) : nullptr, gnext, B * C, dt, stream);
    }
    // the reductions of both weight gradients ride in front of the input-gradient kernel's launch (cfd_tail.h); whatever
    // a producer could not defer it has already reduced itself.  The 1x1 weight gradient needs only gcur and a_l; with
    // side_stream bit 2 it runs on the side stream (side.cpp) beside the transform and the mode-domain kernel.  OFF by default:
    // measured (profiles/r04a_side_stream_ab.txt) the two do run concurrently, but the latency-bound mode-domain kernel then
    // takes 53 us instead of 26 -- it needs the wave slots the streaming kernel occupies -- and the phase is no shorter.
    hipStream_t side = cfd_side_fork((hipStream_t)stream, 2);
    CfdReduceTail tail{};
    CFD_TRY(cfd_int_chan_wgrad(gcur, (const float*)v.act(l), g->w0_w[l], g->w0_b[l], v.scratch2(), B, C, C, HWp, act, side, &tail.chan));
    CFD_TRY(cfd_spectral_dft(p, gcur, v.gh(), B * C, 0, stream));
    CFD_TRY(cfd_int_spectral_mix_adj_wgrad(p, v.xh(l), v.gh(), prm->spec_w1[l], prm->spec_w2[l], v.z(), g->spec_w1[l], g->spec_w2[l], v.scratch(),
                                           B, C, C, stream, &tail.spec));
    CFD_TRY(cfd_side_join((hipStream_t)stream, side));  // the block kernel reduces the 1x1 partial sums
    if (rt.head && phase == 1)  // the reduction cfd_fno_forward_train_f left behind (records at head_rec: nothing of this phase touched them)
        tail.head = cfd_int_head_tail(v.head_rec(), g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, sums, B, C, s->out_chan, HW,
                                      rt.scale ? (float)((double)B * s->out_chan * HW) : 0.f);
    tail.nblk = (tail.spec.part || tail.chan.part || tail.head.part) ? 128 : 0;
    const CfdStemG sg{(l == 0 && rt.stemg) ? inputs : nullptr, mask, p->d_gx, p->d_gy, v.stem_part(), s->in_chan};
    return cfd_int_fno_block_bwd_input(p, gcur, v.z(), prm->w0_w[l], act ? (const float*)v.act(l) : nullptr, gnext, B, C, C, stream, &tail, &sg);
}

extern "C" int cfd_fno_backward(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm,
                                const cfd_fno_params* g, const float* inputs, const float* case_params,
                                const float* mask, const float* label, const float* preds, const float* gpreds_ext,
                                const float* coef, void* ws, void* stream) {
    CFD_TRY(check_shape("cfd_fno_backward", p, s));
    for (int phase = 0; phase <= s->num_layers + 1; ++phase)
        CFD_TRY(cfd_fno_backward_phase(p, s, prm, g, inputs, case_params, mask, label, preds, gpreds_ext, coef, ws, phase,
                                       stream));
    return CFD_OK;
}

// The optimiser launch of the fused training step: Adam over the flat buffers, the deferred nMSE normaliser (sums[3] / sums[2] on top of
// grad_scale) and the lifting layer's gradient rows (see include/cfdbench_amd.h).  `params` / `grads` point into `param` / `grad`.
// cfd_fno_adam_step_ema: the same call with an exponential moving average of the parameters kept inside the optimiser launch
// (ema == NULL: cfd_fno_adam_step itself, which forwards here).
extern "C" int cfd_fno_adam_step(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm, const cfd_fno_params* g,
                                 const float* inputs, const float* case_params, const float* mask, const float* sums, void* ws,
                                 float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, float grad_scale, int which, int act_dtype,
                                 int flags, void* stream) {
    return cfd_fno_adam_step_ema(p, s, prm, g, inputs, case_params, mask, sums, ws, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                                 weight_decay, step, grad_scale, which, act_dtype, flags, stream, nullptr, 0.f);
}

extern "C" int cfd_fno_adam_step_ema(const cfd_plan* p, const cfd_fno_shape* s, const cfd_fno_params* prm, const cfd_fno_params* g,
                                     const float* inputs, const float* case_params, const float* mask, const float* sums, void* ws,
                                     float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, int step, float grad_scale, int which, int act_dtype,
                                     int flags, void* stream, float* ema, float ema_decay) {
    CFD_TRY(check_shape("cfd_fno_adam_step", p, s, act_dtype));
    CFD_REQUIRE(prm && g && ws && param && grad, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: NULL pointer");
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || act_dtype == CFD_DT_BF16, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: act_dtype %d", act_dtype);
    // CFD_STEP_ACCUMULATE: `param` is an accumulator laid out like `grad`; the call finishes the pass's gradient and adds it instead of
    // running Adam (the moments, the hyper-parameters and grads->clip are not read)
    const bool accumulate = (flags & CFD_STEP_ACCUMULATE) != 0;
    CFD_REQUIRE(accumulate || !(flags & CFD_STEP_ACCUM_INIT), CFD_ERR_INVALID_ARG,
                "cfd_fno_adam_step: CFD_STEP_ACCUM_INIT without CFD_STEP_ACCUMULATE");
    if (accumulate && n == 0) return CFD_OK;  // (an empty accumulator: nothing to finish, nothing to add)
    // grads->clip / max_grad_norm (ABI 604) are read here and nowhere else: the route does not depend on them
    CFD_REQUIRE(accumulate || !g->clip || g->max_grad_norm > 0.f, CFD_ERR_INVALID_ARG,
                "cfd_fno_adam_step: grads->max_grad_norm must be > 0 when grads->clip is set (+inf: measure the norm, clip nothing)");
    // CFD_STEP_SKIP_NONFINITE: the optimiser call skips a step whose gradient norm is not finite.  The norm is the clip buffer's, so the
    // bit needs it; with CFD_STEP_ACCUMULATE no norm is taken and the bit is ignored (the guard fires later, on the accumulator)
    const bool guard = !accumulate && (flags & CFD_STEP_SKIP_NONFINITE) != 0;
    // the average follows the parameters: an accumulate call writes none, so it ignores both arguments.  (The test is written so that a
    // NaN decay fails it.)
    if (accumulate) ema = nullptr;
    CFD_REQUIRE(!ema || (ema_decay >= 0.f && ema_decay < 1.f), CFD_ERR_INVALID_ARG,
                "cfd_fno_adam_step_ema: ema_decay must be >= 0 and < 1 (got %g)", (double)ema_decay);
    CFD_REQUIRE(!guard || g->clip, CFD_ERR_INVALID_ARG,
                "cfd_fno_adam_step: CFD_STEP_SKIP_NONFINITE needs grads->clip (max_grad_norm = +inf: guard without clipping)");
    const View v(p, s, 1, act_dtype, ws);
    CFD_REQUIRE(act_dtype == CFD_DT_F32 || !wants_ingrad(g), CFD_ERR_UNSUPPORTED,
                "cfd_fno_adam_step: grads->d_inputs / d_case_params need fp32 activation storage");
    const Route rt = route(p, s, v, which, act_dtype, flags, inputs, mask, g);
    CFD_REQUIRE(!rt.scale || sums, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: CFD_TRAIN_DEFER_SCALE needs the `sums` of the forward call");
    StemAdamJob job{};
    if (rt.stem) {
        CFD_REQUIRE(case_params || s->n_case_params == 0, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: NULL case_params");
        const float* gw = (const float*)g->fc0_w;
        const float* gb = (const float*)g->fc0_b;
        CFD_REQUIRE(gw >= grad && gb >= grad && (size_t)(gw - grad) < n && (size_t)(gb - grad) < n, CFD_ERR_INVALID_ARG,
                    "cfd_fno_adam_step: grads->fc0 does not point into the flat gradient buffer");
        CFD_REQUIRE((const float*)prm->fc0_w - param == gw - grad && (const float*)prm->fc0_b - param == gb - grad, CFD_ERR_INVALID_ARG,
                    "cfd_fno_adam_step: params and grads are laid out differently");
        const size_t w_end = (size_t)(gw - grad) + (size_t)s->hidden * (s->in_chan + 3 + s->n_case_params), b_end = (size_t)(gb - grad) + s->hidden;
        CFD_REQUIRE(!accumulate || (w_end <= n && b_end <= n), CFD_ERR_INVALID_ARG,
                    "cfd_fno_adam_step: grads->fc0 reaches past the flat gradient buffer");
        const int spl = cfd_int_stemg_splits(p, s->B);
        job = StemAdamJob{v.stem_part(), case_params, s->B * spl, spl, s->n_case_params, s->in_chan, s->hidden, (long)(gw - grad), (long)(gb - grad)};
    }
    if (accumulate)
        return cfd_int_grad_accum_f(param, grad, n, grad_scale, rt.scale ? sums : nullptr, rt.stem ? &job : nullptr,
                                    (flags & CFD_STEP_ACCUM_INIT) != 0, stream);
    return cfd_int_adam_flat_f(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                               rt.scale ? sums : nullptr, rt.stem ? &job : nullptr, g->clip, g->max_grad_norm,
                               (flags & CFD_STEP_DECOUPLED_WD) != 0, guard, ema, ema_decay, stream);
}
