// READ's MIMO-UNet-style refinement CNN (READ/models/unet.py:121-285) as a pre-built launch plan.
//
// The network is fixed by the reference (get_net(): UNet(8, 3, feature_scale=4, num_res=4),
// READ/pipelines/ogl.py:19-27; base_channel 32, unet.py:141), so the plan is built once per
// resolution: 99 fused gated-conv launches (+ 3 for the AFF inputs of coarser levels) + 3 bilinear x4 upsamples, every torch.cat /
// F.interpolate(nearest) / FAM multiply / residual add folded into a conv's loader or epilogue.
// Activations are NHWC fp32 in a caller-provided workspace; one C-ABI call enqueues a frame.
#include <math.h>

#include <string>
#include <vector>

#include "common.h"
#include "internal.h"

using namespace readhip;

namespace {

constexpr int BASE = 32;      // base_channel, unet.py:141
constexpr int NUM_RES = 4;    // num_res, ogl.py:24
constexpr int IN_CH = READ_DESC_CHANNELS;

// A weight order is one packed form of a layer's weights: what one kernel family reads.  One row per order, in the sequence the
// packed blob carries them; everything below that places, packs or hands out an order walks this table.
enum Order { DIRECT, WINO, W16, W4, W4H, F4X1, DKH, T3H, SC, N_ORDERS };
constexpr size_t ABSENT = ~(size_t)0;      // an offset of an order the layer does not carry

template <auto F> size_t floats2(int cin, int cout, int) { return F(cin, cout); }      // size functions and packers without ksize / kc
template <auto F> int pack2(int cin, int cout, int, int, const float *wf, const float *wm, float *dst) { return F(cin, cout, wf, wm, dst); }
int pack_dkh(int cin, int cout, int k, int, const float *wf, const float *wm, float *dst) { return read_conv_pack_dkh_host(cin, cout, k, wf, wm, dst); }

const struct OrderRow {
    const char *name;
    size_t (*floats)(int cin, int cout, int k);
    int (*pack)(int cin, int cout, int k, int kc, const float *wf, const float *wm, float *dst);
    size_t align;                          // of its offset in the blob, in floats
    const float *read_conv_desc::*field;   // the read_conv_desc pointer it fills (the f16 operands are declared const void *) ...
    const void *read_conv_desc::*field_h;  // ... both null: the order travels beside the descriptor, whose struct is frozen
} ORDERS[N_ORDERS] = {
    {"direct", read_conv_packed_floats, read_conv_pack_weights_host, 1, &read_conv_desc::wpacked, nullptr},
    {"wino", floats2<read_conv_wino_floats>, pack2<read_conv_pack_wino_host>, 1, &read_conv_desc::wpacked_wino, nullptr},
    {"w16", floats2<read_conv_wino_floats>, pack2<read_conv_pack_w16_host>, 1, &read_conv_desc::wpacked_w16, nullptr},
    {"w4", floats2<read_conv_w4_floats>, pack2<read_conv_pack_w4_host>, 1, &read_conv_desc::wpacked_w4, nullptr},
    {"w4h", floats2<read_conv_w4h_floats>, pack2<read_conv_pack_w4h_host>, 1, nullptr, &read_conv_desc::wpacked_w4h},
    {"f4x1", floats2<read_conv_f4x1_floats>, pack2<read_conv_pack_f4x1_host>, 1, nullptr, nullptr},
    {"dkh", read_conv_dkh_floats, pack_dkh, 1, nullptr, &read_conv_desc::wpacked_d3h},
    {"t3h", floats2<read_conv_t3h_floats>, pack2<read_conv_pack_t3h_host>, 1, nullptr, &read_conv_desc::wpacked_t3h},
    {"sc", floats2<read_conv_sc_floats>, pack2<read_conv_pack_sc_host>, 16, &read_conv_desc::wpacked_sc, nullptr},   // 64 bytes: scalar loads of 16 dwords
};

// A convolution of the plan: a BasicConv of the model (LayerInfo) or a 1x1 block cut out of some (DerivedInfo).
struct ConvInfo {
    std::string path;
    int cin, cout, k, stride, elu, kc;
    size_t p_off = 0;                      // float offset of the parameters in the packed blob
    size_t off[N_ORDERS];                  // ... of each weight order, or ABSENT
    size_t side_off = ABSENT;              // FULL layout: offset of the F4X1 order in the side buffer (read_unet_set_f4x1), else ABSENT
    ConvInfo(const std::string &path, int cin, int cout, int k, int stride, int elu, int kc)
        : path(path), cin(cin), cout(cout), k(k), stride(stride), elu(elu), kc(kc)
    {
        for (size_t &o : off) o = ABSENT;
    }
};

struct LayerInfo : ConvInfo {
    using ConvInfo::ConvInfo;
    size_t raw_off = 0;                    // float offset into the raw blob
};

// A 1x1 layer whose weights are a block of existing layers' weights: input channels [ci0, ci0 + cin) of the parts'
// concatenated input, the parts' output channels stacked.  Used to evaluate the coarse-level inputs of the AFF 1x1
// convs at their own resolution (a 1x1 conv commutes with the nearest up-sampling of unet.py:239-254).  Its parameters
// are zero biases — gated finals use their part's own p_off.
struct DerivedInfo : ConvInfo {
    using ConvInfo::ConvInfo;
    int ci0 = 0;
    std::vector<int> parts;                // indices into Arch::layers
};

enum Home { NOWHERE, BLOB, SIDE };

// Layout of the packed blob.  FULL: every fragment order of every layer (direct + both F(2x2) orders + F(4x4) where they exist):
// any tuning knob can send a layer to any of its kernels — 952 MB for a 121 MB model.  LEAN: what the default plan reads —
// a layer the F(4x4) kernel takes carries its F(4x4) order ONLY (that kernel runs 73 of the 105 launches; its layers' other three
// orders were 500 MB nobody touched), the layers no launch executes (ConvsOut) carry nothing; everything else as in FULL.
// The raw blob (read_unet_raw_floats) is the same for both.
// The F(4,3)-by-rows order of the split-operand 3x3/s1 layers (gated_conv_f4x1h_kernel, which runs them by default): LEAN carries it
// behind the F(4x4) split operand of each such layer (both, so read_tuning_set("conv_f4x1", 0) still works on it); FULL is laid out
// exactly as before — a host derives the order from FULL's direct fragments (exact weights) and hands it over as a side buffer
// (read_unet_f4x1_layer / read_unet_set_f4x1).  LEAN_W4H is the lean layout without it: blobs packed before the kernel existed.
// One rule per order, asked in the blob's sequence: does this convolution carry the order in this layout, and where.
Home home(Order o, const ConvInfo &L, int layout)
{
    const bool lean = layout != READ_UNET_LAYOUT_FULL;
    const bool k3s1 = L.k == 3 && L.stride == 1;
    const bool unused = L.path.compare(0, 9, "ConvsOut.") == 0;                  // no launch executes these layers
    const bool fam = L.path.compare(0, 3, "FAM") == 0;                           // x1 * x2 launches: the DIRECT split-operand kernel takes them
    const bool wino = k3s1 && L.kc == 16 && L.cin % 16 == 0;
    const bool w4 = wino && L.cin >= 32 && L.cout % 32 == 0;                     // the F(4x4) family runs the layer by default ...
    const bool split = w4 && L.cin % 32 == 0;                                    // ... with split operands on the f16 matrix cores
    const bool s2 = (L.k == 3 || L.k == 4) && L.stride == 2 && L.cin % 32 == 0 && L.cout % 32 == 0;   // down-sampling (3x3) and decoder (4x4) layers: direct split-operand kernel
    bool in = false;
    switch (o) {
    case DIRECT: in = !(lean && (w4 || unused || s2)); break;                    // lean: absent where a split-operand or F(4x4) kernel runs the layer
    case WINO:
    case W16: in = wino && !(lean && (w4 || unused)); break;
    case W4: in = w4 && !(lean && split); break;
    case W4H: in = split && !fam; break;
    case F4X1: in = split && !fam && layout != READ_UNET_LAYOUT_LEAN_W4H; break;   // the W4H layers; LEAN_W4H predates the order
    case DKH:                                                                    // 1x1 layers: the fp32 order stays beside it as the fallback
        in = (split && (fam || !lean)) || s2 || (L.k == 1 && L.stride == 1 && L.cin <= 256);
        break;
    case T3H: in = k3s1 && L.cin == IN_CH; break;                                // over the 8-channel pyramid
    case SC: in = k3s1 && !(lean && unused); break;                              // Cout <= 4: the output layer
    default: break;
    }
    if (!in || !ORDERS[o].floats(L.cin, L.cout, L.k)) return NOWHERE;            // a size function answers 0 for a shape its kernel does not take
    // FULL is laid out as it was before F4X1 existed: a host derives that order from the direct fragments into a side buffer
    return o == F4X1 && !lean ? SIDE : BLOB;
}

struct Arch {
    std::vector<LayerInfo> layers;
    std::vector<DerivedInfo> derived;
    size_t raw_floats = 0, packed_floats = 0, side_floats = 0;
    int find_derived(const std::string &p) const
    {
        for (size_t i = 0; i < derived.size(); ++i)
            if (derived[i].path == p) return (int)i;
        return -1;
    }
    int find(const std::string &p) const
    {
        for (size_t i = 0; i < layers.size(); ++i)
            if (layers[i].path == p) return (int)i;
        return -1;
    }
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t raw_layer_floats(int cin, int cout, int k) { return 2 * ((size_t)cout * cin * k * k + cout) + 4 * (size_t)cout; }

Arch build_arch(int layout)
{
        Arch a;
        // the blob's sequence: a layer's parameters, then its orders in table order; a derived layer's direct order, parameters, the rest
        auto params = [&](ConvInfo &L) {
            L.p_off = a.packed_floats;
            a.packed_floats += read_conv_param_floats(L.cout);
        };
        auto place = [&](ConvInfo &L, int first, int last) {
            for (int o = first; o <= last; ++o) {
                const Home h = home((Order)o, L, layout);
                const size_t n = ORDERS[o].floats(L.cin, L.cout, L.k);
                if (h == BLOB) {
                    L.off[o] = a.packed_floats = align_up(a.packed_floats, ORDERS[o].align);
                    a.packed_floats += n;
                } else if (h == SIDE) {
                    L.side_off = a.side_floats;
                    a.side_floats += n;
                }
            }
        };
        auto add = [&](const std::string &path, int cin, int cout, int k, int s, int elu, int kc) {
            LayerInfo L(path, cin, cout, k, s, elu, kc);
            L.raw_off = a.raw_floats;
            a.raw_floats += raw_layer_floats(cin, cout, k);
            params(L);
            place(L, DIRECT, SC);
            a.layers.push_back(L);
        };
        // SCM (unet.py:92-106): SCM2 -> 64 planes @1/2, SCM1 -> 128 @1/4, SCM0 -> 256 @1/8
        const int scm_planes[3] = {BASE * 8, BASE * 4, BASE * 2};   // SCM0, SCM1, SCM2
        for (int n = 0; n < 3; ++n) {
            const int P = scm_planes[n];
            const std::string p = "SCM" + std::to_string(n);
            add(p + ".main.0", IN_CH, P / 4, 3, 1, 1, 8);
            add(p + ".main.1", P / 4, P / 2, 1, 1, 1, 16);
            add(p + ".main.2", P / 2, P / 2, 3, 1, 1, 16);
            add(p + ".main.3", P / 2, P - IN_CH, 1, 1, 1, 16);
            add(p + ".conv", P, P, 1, 1, 0, 8);                     // cat[x(8), main(P-8)]
        }
        // feat_extract (unet.py:156-165)
        add("feat_extract.0", IN_CH, BASE, 3, 1, 1, 8);
        add("feat_extract.1", BASE, BASE * 2, 3, 2, 1, 16);
        add("feat_extract.2", BASE * 2, BASE * 4, 3, 2, 1, 16);
        add("feat_extract.3", BASE * 4, BASE * 2, 4, 2, 1, 16);
        add("feat_extract.4", BASE * 2, BASE, 4, 2, 1, 16);
        add("feat_extract.5", BASE, 3, 3, 1, 0, 16);
        add("feat_extract.6", BASE * 4, BASE * 8, 3, 2, 1, 16);
        add("feat_extract.7", BASE * 8, BASE * 4, 4, 2, 1, 16);
        // Encoder / Decoder: 4 blocks x NUM_RES ResBlocks x 2 BasicConvs (unet.py:11-20,56-76)
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < NUM_RES; ++j) {
                const int C = BASE << i;
                const std::string p = "Encoder." + std::to_string(i) + ".layers." + std::to_string(j) + ".main.";
                add(p + "0", C, C, 3, 1, 1, 16);
                add(p + "1", C, C, 3, 1, 0, 16);
            }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < NUM_RES; ++j) {
                const int C = (BASE * 8) >> i;
                const std::string p = "Decoder." + std::to_string(i) + ".layers." + std::to_string(j) + ".main.";
                add(p + "0", C, C, 3, 1, 1, 16);
                add(p + "1", C, C, 3, 1, 0, 16);
            }
        add("Convs.0", BASE * 8, BASE * 4, 1, 1, 1, 16);
        add("Convs.1", BASE * 4, BASE * 2, 1, 1, 1, 16);
        add("Convs.2", BASE * 2, BASE, 1, 1, 1, 16);
        add("ConvsOut.0", BASE * 4, 3, 3, 1, 0, 16);   // never executed (unet.py:181-186)
        add("ConvsOut.1", BASE * 2, 3, 3, 1, 0, 16);
        for (int i = 0; i < 3; ++i) {
            const std::string p = "AFFs." + std::to_string(i) + ".conv.";
            add(p + "0", BASE * 15, BASE << i, 1, 1, 1, 16);
            add(p + "1", BASE << i, BASE << i, 3, 1, 0, 16);
        }
        add("FAM0.merge", BASE * 8, BASE * 8, 3, 1, 0, 16);
        add("FAM1.merge", BASE * 4, BASE * 4, 3, 1, 0, 16);
        add("FAM2.merge", BASE * 2, BASE * 2, 3, 1, 0, 16);
        // AFF first convs split by the level their inputs live at; concat order res1(32) res2(64) res3(128) z(256)
        auto derive = [&](const std::string &name, int ci0, int cin, const std::vector<std::string> &layers) {
            DerivedInfo D(name, cin, 0, 1, 1, a.layers[a.find(layers[0])].elu, 16);
            D.ci0 = ci0;
            for (const std::string &l : layers) {
                D.parts.push_back(a.find(l));
                D.cout += a.layers[D.parts.back()].cout;
            }
            place(D, DIRECT, DIRECT);
            params(D);
            place(D, DIRECT + 1, SC);
            a.derived.push_back(D);
        };
        const std::string aff0 = "AFFs.0.conv.0", aff1 = "AFFs.1.conv.0", aff2 = "AFFs.2.conv.0";
        derive("AFFq3", BASE * 7, BASE * 8, {aff0, aff1, aff2});   // z    @1/8 -> partial sums of AFF0, AFF1, AFF2
        derive("AFFq2", BASE * 3, BASE * 4, {aff0, aff1});         // res3 @1/4 -> AFF0, AFF1
        derive("AFFq1", BASE, BASE * 2, {aff0});                   // res2 @1/2 -> AFF0
        derive("AFFs.0.conv.0r", 0, BASE, {aff0});                 // what is left at the layer's own level
        derive("AFFs.1.conv.0r", 0, BASE * 3, {aff1});
        derive("AFFs.2.conv.0r", 0, BASE * 7, {aff2});
        // Convs.k = 1x1 over cat[Upsample4_bilinear(fe), r] (unet.py:261-262,269-270,277-278): the half that multiplies the up-sampled
        // tensor is applied at ITS level (1/16 of the pixels, `linear`) and enters the gated launch as a bilinear pre-activation addend
        for (int k = 0; k < 3; ++k) {
            const int Cu = (BASE * 4) >> k;                                  // channels of up4(fe) = channels of r
            const std::string L = "Convs." + std::to_string(k);
            derive(L + ".u", 0, Cu, {L});
            derive(L + ".r", Cu, Cu, {L});
        }
        return a;
}

const Arch &arch(int layout = READ_UNET_LAYOUT_FULL)
{
    static const Arch A[3] = {build_arch(READ_UNET_LAYOUT_FULL), build_arch(READ_UNET_LAYOUT_LEAN), build_arch(READ_UNET_LAYOUT_LEAN_W4H)};
    return A[layout >= 0 && layout < 3 ? layout : 0];
}

// ------------------------------------------------------------------------------------------
struct Tensor {
    std::string name;
    float *p = nullptr;   // null for external tensors until forward()
    int ext = -1;         // 0..3 = x0..x3, 4 = rgb output
    int H = 0, W = 0, C = 0;
};

struct Op {
    enum Kind { CONV, UP4 } kind;
    read_conv_desc d;          // CONV
    const void *wp_f4x1 = nullptr;   // CONV: the F(4,3)-by-rows order of the layer, beside the descriptor (its struct is frozen), or null
    size_t side_off = ~(size_t)0;    // CONV, FULL layout: where that order lies in the side buffer of read_unet_set_f4x1
    int src_t[READ_CONV_MAX_SRC], mul_t, res_t, out_t;   // tensor ids (for external patching)
    int in_t;                  // UP4
    int pre_t = -1;            // CONV: tensor of the pre-activation addend
    double flops;
    int is_c3s1;
    std::string label;
};

}  // namespace

struct read_unet {
    int H, W;
    int layout = READ_UNET_LAYOUT_FULL;
    const float *packed;
    char *ws;
    size_t ws_bytes, ws_used;
    std::vector<Tensor> tensors;
    std::vector<Op> ops;
    hipEvent_t *events = nullptr;
    int n_events = 0;
};

namespace {

int g_unet_aff_split = 1;     // read_tuning_set("unet_aff_split", 0): the AFF first convs as single 480-channel launches
// read_tuning_set("unet_up_fold", 1): the bilinear x4 up-sampling folded into the Convs.k launches (read_conv_desc.pre_bilinear).
// Built and measured in round 5 (profiles/r5_up_fold_ab.md): results equal (148 dB either way) and 110 MB per frame less written and
// re-read, but NOT faster — the three tiny `Convs.k.u` launches cost 14 - 22 us each (launch floor of the 1x1 kernels) and the
// bilinear epilogue gathers 32 float4 per lane: Convs.0 / 1 / 2 take 64.8 / 63.6 / 102.0 us folded against 61.6 / 70.2 / 83.9 with
// the separate pass (non-family launches 1.346 vs 1.332 ms per frame, 220.8 vs 220.4 frames/s).  Default off.
int g_unet_up_fold = 0;

struct Builder {
    read_unet *u;
    bool dry;                   // size-only pass
    size_t used = 0;

    int tensor(const std::string &name, int level, int C)
    {
        Tensor t;
        t.name = name;
        t.H = u->H >> level;
        t.W = u->W >> level;
        t.C = C;
        const size_t bytes = align_up((size_t)t.H * t.W * C * sizeof(float), 256);
        if (!dry) t.p = reinterpret_cast<float *>(u->ws + used);
        used += bytes;
        u->tensors.push_back(t);
        return (int)u->tensors.size() - 1;
    }
    int external(const std::string &name, int ext, int level, int C)
    {
        Tensor t;
        t.name = name;
        t.ext = ext;
        t.H = u->H >> level;
        t.W = u->W >> level;
        t.C = C;
        u->tensors.push_back(t);
        return (int)u->tensors.size() - 1;
    }

    struct PreRef {
        int t = -1, f_off = 0, m_off = 0, shift = 0, bilinear = 0;
    };

    // One BasicConv.  srcs = {tensor id, shift}; out tensor must already exist.
    void conv(const std::string &path, std::vector<std::pair<int, int>> srcs, int out_t, int mul_t = -1,
              int res_t = -1)
    {
        const Arch &A = arch(u->layout);
        const LayerInfo &L = A.layers[A.find(path)];
        emit(L, L.p_off, srcs, out_t, mul_t, res_t, 0, PreRef());
    }
    // A derived 1x1 layer (DerivedInfo): `linear` ones store the pre-activations [f | m] for a finer level to add,
    // gated ones are the AFF layer itself on the inputs of its own level, with the layer's own bias / BatchNorm.
    void conv_derived(const std::string &name, std::vector<std::pair<int, int>> srcs, int out_t, int linear, PreRef pre)
    {
        const Arch &A = arch(u->layout);
        const DerivedInfo &D = A.derived[A.find_derived(name)];
        emit(D, linear ? D.p_off : A.layers[D.parts[0]].p_off, srcs, out_t, -1, -1, linear, pre);
    }

    void emit(const ConvInfo &L, size_t p_off, const std::vector<std::pair<int, int>> &srcs, int out_t, int mul_t, int res_t, int linear,
              PreRef pre)
    {
        Op op;
        memset(&op.d, 0, sizeof(op.d));
        op.kind = Op::CONV;
        op.label = L.path;
        op.mul_t = mul_t;
        op.res_t = res_t;
        op.out_t = out_t;
        op.in_t = -1;
        op.pre_t = pre.t;
        for (int i = 0; i < READ_CONV_MAX_SRC; ++i) op.src_t[i] = -1;
        const Tensor &o = u->tensors[out_t];
        op.d.n_src = (int)srcs.size();
        int cin = 0;
        for (size_t i = 0; i < srcs.size(); ++i) {
            const Tensor &t = u->tensors[srcs[i].first];
            op.src_t[i] = srcs[i].first;
            op.d.src[i].data = t.p;
            op.d.src[i].C = t.C;
            op.d.src[i].srcH = t.H;
            op.d.src[i].srcW = t.W;
            op.d.src[i].shift = srcs[i].second;
            cin += t.C;
        }
        op.d.inH = o.H * L.stride;
        op.d.inW = o.W * L.stride;
        op.d.Cout = L.cout;
        op.d.ksize = L.k;
        op.d.stride = L.stride;
        op.d.elu = L.elu;
        op.d.params = u->packed + p_off;
        for (int r = 0; r < N_ORDERS; ++r) {                      // an order the layout does not carry for this layer: a null pointer
            const float *p = L.off[r] != ABSENT ? u->packed + L.off[r] : nullptr;
            if (ORDERS[r].field) op.d.*ORDERS[r].field = p;
            else if (ORDERS[r].field_h) op.d.*ORDERS[r].field_h = p;
            else op.wp_f4x1 = p;
        }
        op.side_off = L.side_off;
        op.d.mul = mul_t >= 0 ? u->tensors[mul_t].p : nullptr;
        op.d.residual = res_t >= 0 ? u->tensors[res_t].p : nullptr;
        op.d.out = o.p;
        op.d.out_cstride = o.C;
        op.d.config = -1;
        op.d.linear = linear;
        if (pre.t >= 0) {
            const Tensor &pt = u->tensors[pre.t];
            op.d.pre = pt.p;
            op.d.pre_cstride = pt.C;
            op.d.pre_f_off = pre.f_off;
            op.d.pre_m_off = pre.m_off;
            op.d.pre_shift = pre.shift;
            op.d.pre_bilinear = pre.bilinear;
            op.d.preH = pt.H;
            op.d.preW = pt.W;
        }
        op.flops = 2.0 * 2.0 * (double)o.H * o.W * L.cout * cin * L.k * L.k;
        op.is_c3s1 = (L.k == 3 && L.stride == 1 && L.cin == L.cout && L.cin >= BASE) ? 1 : 0;
        if (cin != L.cin) set_error("internal: layer %s expects Cin=%d, plan gives %d", L.path.c_str(), L.cin, cin);
        if (o.C != (linear ? 2 : 1) * L.cout && o.ext < 0)
            set_error("internal: layer %s writes %d channels into a %d-channel tensor", L.path.c_str(), (linear ? 2 : 1) * L.cout, o.C);
        u->ops.push_back(op);
    }
    void up4(int in_t, int out_t)
    {
        Op op;
        memset(&op.d, 0, sizeof(op.d));
        op.kind = Op::UP4;
        op.label = "up4(" + u->tensors[in_t].name + ")";
        op.in_t = in_t;
        op.out_t = out_t;
        op.mul_t = op.res_t = -1;
        for (int i = 0; i < READ_CONV_MAX_SRC; ++i) op.src_t[i] = -1;
        op.flops = 0;
        op.is_c3s1 = 0;
        u->ops.push_back(op);
    }

    // 4 ResBlocks: x + BC1(BC0(x))  (unet.py:11-20); returns the tensor id holding the result.
    int resblocks(const std::string &prefix, int x, int level, int C)
    {
        int t = tensor(prefix + ".t", level, C);
        int y = tensor(prefix + ".y", level, C);
        int spare = tensor(prefix + ".y2", level, C);
        for (int j = 0; j < NUM_RES; ++j) {
            const std::string p = prefix + ".layers." + std::to_string(j) + ".main.";
            conv(p + "0", {{x, 0}}, t);
            conv(p + "1", {{t, 0}}, y, -1, x);
            // rotate: the block input may be needed later only for j == 0 (never overwritten:
            // `spare` takes its place in the ring)
            const int nx = y;
            y = (j == 0) ? spare : x;
            x = nx;
        }
        return x;
    }

    int scm(int n, int xin, int level)
    {
        const int P = (n == 0) ? BASE * 8 : (n == 1 ? BASE * 4 : BASE * 2);
        const std::string p = "SCM" + std::to_string(n);
        int a = tensor(p + ".a", level, P / 4);
        int b = tensor(p + ".b", level, P / 2);
        int c = tensor(p + ".c", level, P / 2);
        int d = tensor(p + ".d", level, P - IN_CH);
        int z = tensor(p + ".out", level, P);
        conv(p + ".main.0", {{xin, 0}}, a);
        conv(p + ".main.1", {{a, 0}}, b);
        conv(p + ".main.2", {{b, 0}}, c);
        conv(p + ".main.3", {{c, 0}}, d);
        conv(p + ".conv", {{xin, 0}, {d, 0}}, z);
        return z;
    }

    void build()
    {
        u->tensors.clear();
        u->ops.clear();
        used = 0;
        const int x0 = external("x0", 0, 0, IN_CH), x1 = external("x1", 1, 1, IN_CH);
        const int x2 = external("x2", 2, 2, IN_CH), x3 = external("x3", 3, 3, IN_CH);
        const int rgb = external("rgb", 4, 0, 3);

        // unet.py:214-216
        const int z2 = scm(2, x1, 1), z4 = scm(1, x2, 2), z8 = scm(0, x3, 3);
        // unet.py:219-220
        int xf = tensor("fe0", 0, BASE);
        conv("feat_extract.0", {{x0, 0}}, xf);
        const int res1 = resblocks("Encoder.0", xf, 0, BASE);
        // unet.py:224-226: z = fe1(res1); z = z + merge(z*z2); res2 = E1(z)
        int f1 = tensor("fe1", 1, BASE * 2), fam2 = tensor("fam2", 1, BASE * 2);
        conv("feat_extract.1", {{res1, 0}}, f1);
        conv("FAM2.merge", {{f1, 0}}, fam2, z2, f1);
        const int res2 = resblocks("Encoder.1", fam2, 1, BASE * 2);
        // unet.py:228-230
        int f2 = tensor("fe2", 2, BASE * 4), fam1 = tensor("fam1", 2, BASE * 4);
        conv("feat_extract.2", {{res2, 0}}, f2);
        conv("FAM1.merge", {{f2, 0}}, fam1, z4, f2);
        const int res3 = resblocks("Encoder.2", fam1, 2, BASE * 4);
        // unet.py:232-235
        int f6 = tensor("fe6", 3, BASE * 8), fam0 = tensor("fam0", 3, BASE * 8);
        conv("feat_extract.6", {{res3, 0}}, f6);
        conv("FAM0.merge", {{f6, 0}}, fam0, z8, f6);
        const int zb = resblocks("Encoder.3", fam0, 3, BASE * 8);

        // unet.py:239-254: nearest resamples folded into the AFF 1x1 convs.
        // shift > 0: source is finer than the destination (down-sampling), < 0: coarser.
        int a0 = tensor("aff0.t", 0, BASE), r1 = tensor("aff0.out", 0, BASE);
        int a1 = tensor("aff1.t", 1, BASE * 2), r2 = tensor("aff1.out", 1, BASE * 2);
        int a2 = tensor("aff2.t", 2, BASE * 4), r3 = tensor("aff2.out", 2, BASE * 4);
        if (g_unet_aff_split) {
            // Every AFF input that lives at a coarser level is multiplied by its weight block AT that level (linear
            // launches q3 -> q2 -> q1, each adding the up-sampled sum of the coarser ones), and the gated layer at the
            // AFF's own level adds the result to its pre-activations: 11.2 instead of 46 GFLOP, same sums re-associated.
            //   q3 = [f0 f1 f2 | m0 m1 m2] (z), q2 = [f0 f1 | m0 m1] (res3 + up q3), q1 = [f0 | m0] (res2 + up q2)
            const int q3 = tensor("aff.q3", 3, 2 * BASE * 7), q2 = tensor("aff.q2", 2, 2 * BASE * 3);
            const int q1 = tensor("aff.q1", 1, 2 * BASE);
            conv_derived("AFFq3", {{zb, 0}}, q3, 1, PreRef());
            conv_derived("AFFq2", {{res3, 0}}, q2, 1, PreRef{q3, 0, BASE * 7, 1});
            conv_derived("AFFs.2.conv.0r", {{res1, 2}, {res2, 1}, {res3, 0}}, a2, 0, PreRef{q3, BASE * 3, BASE * 10, 1});
            conv_derived("AFFq1", {{res2, 0}}, q1, 1, PreRef{q2, 0, BASE * 3, 1});
            conv_derived("AFFs.1.conv.0r", {{res1, 1}, {res2, 0}}, a1, 0, PreRef{q2, BASE, BASE * 4, 1});
            conv_derived("AFFs.0.conv.0r", {{res1, 0}}, a0, 0, PreRef{q1, 0, BASE, 1});
        } else {
            conv("AFFs.0.conv.0", {{res1, 0}, {res2, -1}, {res3, -2}, {zb, -3}}, a0);
            conv("AFFs.1.conv.0", {{res1, 1}, {res2, 0}, {res3, -1}, {zb, -2}}, a1);
            conv("AFFs.2.conv.0", {{res1, 2}, {res2, 1}, {res3, 0}, {zb, -1}}, a2);
        }
        conv("AFFs.0.conv.1", {{a0, 0}}, r1);
        conv("AFFs.1.conv.1", {{a1, 0}}, r2);
        conv("AFFs.2.conv.1", {{a2, 0}}, r3);

        // unet.py:257-265
        int z = resblocks("Decoder.0", zb, 3, BASE * 8);
        // Convs.k over cat[Upsample4(fe), r]: with unet_up_fold the up-sampled tensor is never written — `Convs.k.u` applies its
        // weight block to fe at fe's level (linear, [f | m]) and `Convs.k.r` adds the bilinear x4 of that to its pre-activations
        auto up_conv = [&](int k, int fe, int level, int C, int r, int out) {
            const std::string L = "Convs." + std::to_string(k);
            if (g_unet_up_fold) {
                const int q = tensor("convs" + std::to_string(k) + ".q", level + 2, 2 * C);
                conv_derived(L + ".u", {{fe, 0}}, q, 1, PreRef());
                conv_derived(L + ".r", {{r, 0}}, out, 0, PreRef{q, 0, C, 2, 1});
            } else {
                const int up = tensor("up" + std::to_string(k), level, C);
                up4(fe, up);
                conv(L, {{up, 0}, {r, 0}}, out);
            }
        };
        int f7 = tensor("fe7", 4, BASE * 4), c0 = tensor("convs0", 2, BASE * 4);
        conv("feat_extract.7", {{z, 0}}, f7);
        up_conv(0, f7, 2, BASE * 4, r3, c0);
        z = resblocks("Decoder.1", c0, 2, BASE * 4);
        // unet.py:268-273
        int f3 = tensor("fe3", 3, BASE * 2), c1 = tensor("convs1", 1, BASE * 2);
        conv("feat_extract.3", {{z, 0}}, f3);
        up_conv(1, f3, 1, BASE * 2, r2, c1);
        z = resblocks("Decoder.2", c1, 1, BASE * 2);
        // unet.py:276-282
        int f4 = tensor("fe4", 2, BASE), c2 = tensor("convs2", 0, BASE);
        conv("feat_extract.4", {{z, 0}}, f4);
        up_conv(2, f4, 0, BASE, r1, c2);
        z = resblocks("Decoder.3", c2, 0, BASE);
        conv("feat_extract.5", {{z, 0}}, rgb);
        u->ws_used = used;
    }
};

int check_hw(int H, int W)
{
    READ_CHECK_ARG(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0,
                   "UNet viewport must be a positive multiple of 16 in both dimensions (got %dx%d)", W, H);
    READ_CHECK_ARG((long long)H * W * BASE * 15 < (1ll << 31), "viewport too large");
    return READ_OK;
}

// Every op goes onto the caller's stream, in plan order.
int run(read_unet *u, const float *const ext[5], int rgb_cstride, hipStream_t s, bool timed)
{
    int ev = 0;
    for (const Op &op : u->ops) {
        if (timed) READ_CHECK_HIP(hipEventRecord(u->events[ev++], s));
        auto ptr = [&](int t) -> const float * {
            if (t < 0) return nullptr;
            const Tensor &T = u->tensors[t];
            return T.ext >= 0 ? ext[T.ext] : T.p;
        };
        if (op.kind == Op::CONV) {
            read_conv_desc d = op.d;
            for (int i = 0; i < d.n_src; ++i) d.src[i].data = ptr(op.src_t[i]);
            d.mul = ptr(op.mul_t);
            d.residual = ptr(op.res_t);
            d.pre = ptr(op.pre_t);
            d.out = const_cast<float *>(ptr(op.out_t));
            if (u->tensors[op.out_t].ext == 4) {
                d.out_cstride = rgb_cstride;
                d.fill_pad = rgb_cstride > d.Cout;   // RGBA: alpha = 1 (READ/gl/nn.py:124)
                d.out_fill = 1.0f;
            }
            const int rc = launch_gated_conv(&d, s, op.wp_f4x1);
            if (rc != READ_OK) return rc;
        } else {
            const Tensor &I = u->tensors[op.in_t];
            const int rc = read_bilinear_up4(ptr(op.in_t), I.H, I.W, I.C, const_cast<float *>(ptr(op.out_t)), s);
            if (rc != READ_OK) return rc;
        }
    }
    if (timed) READ_CHECK_HIP(hipEventRecord(u->events[ev++], s));
    return READ_OK;
}

}  // namespace

extern "C" int read_unet_layer_count(void) { return (int)arch().layers.size(); }

extern "C" int read_unet_layer_info(int i, const char **path, int *cin, int *cout, int *ksize, int *stride, int *elu)
{
    const Arch &A = arch();
    READ_CHECK_ARG(i >= 0 && i < (int)A.layers.size(), "read_unet_layer_info: index %d out of range", i);
    const LayerInfo &L = A.layers[i];
    if (path) *path = L.path.c_str();
    if (cin) *cin = L.cin;
    if (cout) *cout = L.cout;
    if (ksize) *ksize = L.k;
    if (stride) *stride = L.stride;
    if (elu) *elu = L.elu;
    return READ_OK;
}

extern "C" size_t read_unet_raw_floats(void) { return arch().raw_floats; }
extern "C" size_t read_unet_packed_floats(void) { return arch().packed_floats; }
extern "C" size_t read_unet_packed_floats_layout(int layout)
{
    return (layout >= READ_UNET_LAYOUT_FULL && layout <= READ_UNET_LAYOUT_LEAN_W4H) ? arch(layout).packed_floats : 0;
}

extern "C" int read_unet_pack_host(const float *raw, float bn_eps, float *packed)
{
    return read_unet_pack_host_layout(raw, bn_eps, packed, READ_UNET_LAYOUT_FULL);
}

extern "C" int read_unet_pack_host_layout(const float *raw, float bn_eps, float *packed, int layout)
{
    READ_CHECK_ARG(raw && packed, "read_unet_pack_host: null pointer");
    READ_CHECK_ARG(layout >= READ_UNET_LAYOUT_FULL && layout <= READ_UNET_LAYOUT_LEAN_W4H, "read_unet_pack_host: unknown layout %d", layout);
    auto pack = [&](const ConvInfo &L, const float *wf, const float *wm) {
        for (int o = 0; o < N_ORDERS; ++o)
            if (L.off[o] != ABSENT) {
                const int rc = ORDERS[o].pack(L.cin, L.cout, L.k, L.kc, wf, wm, packed + L.off[o]);
                if (rc) return rc;
            }
        return (int)READ_OK;
    };
    for (const LayerInfo &L : arch(layout).layers) {
        const size_t wn = (size_t)L.cout * L.cin * L.k * L.k;
        const float *wf = raw + L.raw_off, *bf = wf + wn, *wm = bf + L.cout, *bm = wm + wn;
        const float *gamma = bm + L.cout, *beta = gamma + L.cout, *mean = beta + L.cout, *var = mean + L.cout;
        int rc = read_conv_pack_params_host(L.cout, bf, bm, gamma, beta, mean, var, bn_eps, packed + L.p_off);
        if (rc) return rc;
        rc = pack(L, wf, wm);
        if (rc) return rc;
    }
    const Arch &A = arch(layout);
    for (const DerivedInfo &D : A.derived) {
        std::vector<float> wf((size_t)D.cout * D.cin), wm(wf.size()), zero(D.cout, 0.0f), one(D.cout, 1.0f);
        int co0 = 0;
        for (int li : D.parts) {
            const LayerInfo &L = A.layers[li];                     // 1x1: weights (cout, cin)
            const float *lf = raw + L.raw_off, *lm = lf + (size_t)L.cout * L.cin + L.cout;
            for (int co = 0; co < L.cout; ++co)
                for (int ci = 0; ci < D.cin; ++ci) {
                    wf[(size_t)(co0 + co) * D.cin + ci] = lf[(size_t)co * L.cin + D.ci0 + ci];
                    wm[(size_t)(co0 + co) * D.cin + ci] = lm[(size_t)co * L.cin + D.ci0 + ci];
                }
            co0 += L.cout;
        }
        int rc = pack(D, wf.data(), wm.data());
        if (rc) return rc;
        rc = read_conv_pack_params_host(D.cout, zero.data(), zero.data(), one.data(), zero.data(), zero.data(), one.data(), 0.0f,
                                        packed + D.p_off);
        if (rc) return rc;
    }
    return READ_OK;
}

extern "C" size_t read_unet_workspace_bytes(int H, int W)
{
    if (check_hw(H, W) != READ_OK) return 0;
    read_unet tmp;
    tmp.H = H;
    tmp.W = W;
    tmp.packed = nullptr;
    tmp.ws = nullptr;
    Builder b{&tmp, true};
    b.build();
    return tmp.ws_used;
}

extern "C" int read_unet_create(read_unet_t **out, const float *packed, int H, int W, void *ws, size_t ws_bytes)
{
    return read_unet_create_layout(out, packed, H, W, ws, ws_bytes, READ_UNET_LAYOUT_FULL);
}

extern "C" int read_unet_create_layout(read_unet_t **out, const float *packed, int H, int W, void *ws, size_t ws_bytes, int layout)
{
    READ_CHECK_ARG(out && packed && ws, "read_unet_create: null pointer");
    READ_CHECK_ARG(layout >= READ_UNET_LAYOUT_FULL && layout <= READ_UNET_LAYOUT_LEAN_W4H, "read_unet_create: unknown layout %d", layout);
    READ_CHECK_ARG((uintptr_t)packed % 16 == 0 && (uintptr_t)ws % 256 == 0, "read_unet_create: misaligned weights/workspace");
    int rc = check_hw(H, W);
    if (rc) return rc;
    const size_t need = read_unet_workspace_bytes(H, W);
    if (ws_bytes < need) {
        set_error("read_unet_create: workspace %zu < %zu bytes", ws_bytes, need);
        return READ_ENOMEM;
    }
    read_unet *u = new read_unet();
    u->H = H;
    u->W = W;
    u->layout = layout;
    u->packed = packed;
    u->ws = (char *)ws;
    u->ws_bytes = ws_bytes;
    set_error("");
    Builder b{u, false};
    b.build();
    // a lean blob serves exactly the launches the F(4x4) kernel takes under the CURRENT tuning state and at THIS size: a knob
    // that sends such a layer elsewhere (conv_w4), or a tensor of 2 GiB and more, needs the full layout
    for (const Op &op : u->ops) {
        const int family = op.kind == Op::CONV && !op.d.wpacked ? conv_family(&op.d) : 4;
        if (family < 4 || family > 6)                               // 4, 5, 6: the F(4x4) family and the direct split-operand kernels
            set_error("read_unet_create: layer %s is not run by the F(4x4) kernel here and the lean blob carries no other fragment "
                      "order for it (pack with READ_UNET_LAYOUT_FULL)", op.label.c_str());
    }
    if (read_last_error()[0]) {   // the builder reports plan inconsistencies through set_error
        delete u;
        return READ_EINVAL;
    }
    *out = u;                     // (nothing here touches a device: the plan can be built without one)
    return READ_OK;
}

// The F(4,3)-by-rows orders of a FULL-layout plan.  The FULL blob is laid out as it always was and does not carry them; it does carry
// every such layer's exact weights (the direct fragment order), so a host derives them once per blob: for j = 0, 1, ... until
// read_unet_f4x1_layer returns non-zero, read_conv_unpack_weights_host(cin, cout, 3, 16, blob + w_off) -> read_conv_pack_f4x1_host
// -> side + side_off; read_unet_f4x1_floats() floats in all.  read_unet_set_f4x1 hands the buffer (device memory that outlives the
// handle) to a plan created from a FULL blob; without it the plan runs those layers on the F(4x4) split-operand kernel.
extern "C" size_t read_unet_f4x1_floats(void) { return arch(READ_UNET_LAYOUT_FULL).side_floats; }

extern "C" int read_unet_f4x1_layer(int j, size_t *w_off, size_t *side_off, int *cin, int *cout)
{
    if (j < 0 || !w_off || !side_off || !cin || !cout) return READ_EINVAL;
    for (const LayerInfo &L : arch(READ_UNET_LAYOUT_FULL).layers)
        if (L.side_off != ABSENT && j-- == 0) {
            *w_off = L.off[DIRECT];
            *side_off = L.side_off;
            *cin = L.cin;
            *cout = L.cout;
            return READ_OK;
        }
    return READ_EINVAL;                                             // past the last layer (no error text: this ends the enumeration)
}

extern "C" int read_unet_set_f4x1(read_unet_t *u, const float *side)
{
    READ_CHECK_ARG(u, "read_unet_set_f4x1: null handle");
    READ_CHECK_ARG(u->layout == READ_UNET_LAYOUT_FULL, "read_unet_set_f4x1: only a plan of the FULL layout takes a side buffer (LEAN carries the order)");
    READ_CHECK_ARG((uintptr_t)side % 16 == 0, "read_unet_set_f4x1: misaligned buffer");
    for (Op &op : u->ops)
        if (op.kind == Op::CONV && op.side_off != ABSENT) op.wp_f4x1 = side ? side + op.side_off : nullptr;
    return READ_OK;
}

extern "C" void read_unet_destroy(read_unet_t *u)
{
    if (!u) return;
    for (int i = 0; i < u->n_events; ++i) (void)hipEventDestroy(u->events[i]);
    delete[] u->events;
    delete u;
}

extern "C" int read_unet_forward(read_unet_t *u, const float *x0, const float *x1, const float *x2,
                                 const float *x3, float *rgb, int rgb_cstride, void *stream)
{
    READ_CHECK_ARG(u && x0 && x1 && x2 && x3 && rgb, "read_unet_forward: null pointer");
    READ_CHECK_ARG(rgb_cstride == 3 || rgb_cstride == 4, "read_unet_forward: rgb_cstride must be 3 or 4");
    const float *ext[5] = {x0, x1, x2, x3, rgb};
    return run(u, ext, rgb_cstride, as_stream(stream), false);
}

extern "C" int read_unet_launch_count(read_unet_t *u) { return u ? (int)u->ops.size() : 0; }

extern "C" int read_unet_profile(read_unet_t *u, const float *x0, const float *x1, const float *x2,
                                 const float *x3, float *rgb, int rgb_cstride, void *stream, float *ms,
                                 double *flops, int *is_conv3x3_s1)
{
    READ_CHECK_ARG(u && x0 && x1 && x2 && x3 && rgb && ms, "read_unet_profile: null pointer");
    READ_CHECK_ARG(rgb_cstride == 3 || rgb_cstride == 4, "read_unet_profile: rgb_cstride must be 3 or 4");
    const int n = (int)u->ops.size();
    if (!u->events) {
        u->events = new hipEvent_t[n + 1];
        for (int i = 0; i <= n; ++i) READ_CHECK_HIP(hipEventCreate(&u->events[i]));
        u->n_events = n + 1;
    }
    const float *ext[5] = {x0, x1, x2, x3, rgb};
    hipStream_t s = as_stream(stream);
    const int rc = run(u, ext, rgb_cstride, s, true);
    if (rc) return rc;
    READ_CHECK_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        READ_CHECK_HIP(hipEventElapsedTime(&ms[i], u->events[i], u->events[i + 1]));
        if (flops) flops[i] = u->ops[i].flops;
        // 0: not in the 3x3/s1 C->C family; else the kernel family that runs it (read_conv_kernel_family: 2 Winograd F(2x2,3x3), 4 F(4x4,3x3),
        //    5 the same with split operands on the f16 matrix cores, 6 direct 3x3 with split operands), 1 for the direct fp32 kernels
        //    (the Winograd kernels spend 2.25x / 4x fewer MFMA flops than `flops`)
        if (is_conv3x3_s1) {
            const int family = u->ops[i].is_c3s1 && u->ops[i].kind == Op::CONV ? conv_family(&u->ops[i].d) : 0;
            is_conv3x3_s1[i] = u->ops[i].is_c3s1 ? (family ? family : 1) : 0;
        }
    }
    return READ_OK;
}

extern "C" int read_unet_launch_info(read_unet_t *u, int i, double *flops, int *is_conv3x3_s1, int *outH, int *outW,
                                     int *cin, int *cout)
{
    READ_CHECK_ARG(u && i >= 0 && i < (int)u->ops.size(), "read_unet_launch_info: bad handle or index");
    const Op &op = u->ops[i];
    const Tensor &o = u->tensors[op.out_t];
    if (flops) *flops = op.flops;
    if (is_conv3x3_s1) *is_conv3x3_s1 = op.is_c3s1;
    if (outH) *outH = o.H;
    if (outW) *outW = o.W;
    int ci = 0;
    for (int k = 0; k < READ_CONV_MAX_SRC; ++k)
        if (op.src_t[k] >= 0) ci += u->tensors[op.src_t[k]].C;
    if (op.kind == Op::UP4) ci = u->tensors[op.in_t].C;
    if (cin) *cin = ci;
    if (cout) *cout = o.C;
    return READ_OK;
}

extern "C" const char *read_unet_launch_label(read_unet_t *u, int i)
{
    return (u && i >= 0 && i < (int)u->ops.size()) ? u->ops[i].label.c_str() : "";
}

extern "C" const float *read_unet_debug_tensor(read_unet_t *u, const char *name, int *H, int *W, int *C)
{
    if (!u || !name) return nullptr;
    for (const Tensor &t : u->tensors)
        if (t.name == name) {
            if (H) *H = t.H;
            if (W) *W = t.W;
            if (C) *C = t.C;
            return t.p;
        }
    return nullptr;
}

namespace readhip {
static const TuneRow k_unet_knobs[] = {
    {"unet_aff_split", &g_unet_aff_split, TN_FLAG, 0, 0},     // 0: AFF first convs as single 480-channel launches (plans created afterwards)
    {"unet_up_fold", &g_unet_up_fold, TN_FLAG, 0, 0},         // 0: Upsample4(bilinear) as a separate pass and Convs.k over the concat (plans created afterwards)
};
constexpr int N_UNET_KNOBS = sizeof(k_unet_knobs) / sizeof(k_unet_knobs[0]);
int unet_set(const char *key, int v) { return tune_set(k_unet_knobs, N_UNET_KNOBS, key, v); }
int unet_get(const char *key, int *value) { return tune_get(k_unet_knobs, N_UNET_KNOBS, key, value); }
const char *unet_key(int i) { return tune_key(k_unet_knobs, N_UNET_KNOBS, i); }
}
