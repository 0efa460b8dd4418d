// Network plan + executor: ingests a reference PosePredictor state_dict by key name, folds
// eval-mode BatchNorm, repacks the weights for the implicit-GEMM kernels, owns the
// activation arena and sequences the launches of one forward pass on a HIP stream.
//
// Reference counterparts: backbone construction MP/training/pose_models_cfg.py:94-122,
// CP/training/pose_models_cfg.py:30-53; forward MP/models/torchvision_resnet.py:325-341,
// MP/models/wide_resnet.py:120-129 (+ BasicBlock :110-126 / BasicBlockV2 :59-65);
// heads MP/models/pose_rigid.py:135-149,352-374, CP/models/pose.py:45-47,108-114.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "conv.h"

namespace hp {

namespace {

const int kLayers34[4] = {3, 4, 6, 3};
const int kLayers18[4] = {2, 2, 2, 2};
const int kPlanes[4] = {64, 128, 256, 512};

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {
    if (p) { (void)hipFree(p); p = nullptr; }
    HP_CHECK_HIP(hipMalloc(&p, bytes ? bytes : 4));
    return HP_OK;
  }
  int upload(const void* h, size_t bytes) {
    int rc = alloc(bytes);
    if (rc) return rc;
    HP_CHECK_HIP(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
    return HP_OK;
  }
};

// which weight sets a layer gets: conv_weight_sets() is the one statement of it
struct WeightSets { bool split, isplit, wino, stem7, shortcut; };

struct ConvLayer {
  std::string wname;       // e.g. "backbone.layer1.0.conv1.weight"
  std::string bn_after;    // BN folded into this conv ("" = none)
  std::string bn_before;   // BN + ReLU applied to the input as prologue ("" = none)
  std::string bias_name;   // the convolution's own bias ("" = none; FPN convs), added to the folded-BN shift
  int cin_real, cin, cout, kh, kw, stride, pad, relu;
  int cout_real = 0;       // rows of the parameter tensor when cout was rounded up to 4 (zero rows; 0 = cout)
  int H, W, Ho, Wo, Kpad;
  int in_buf, out_buf, res_buf;  // arena slots; -1 = network input / none
  DevBuf w_short;  // a 1x1 / stride-2 shortcut in the centre of a zero 3x3 filter, split like a stride-2 3x3 layer's weights: it runs as
                   // extra work items of the block's 3x3 / stride-2 launch (ConvArgs::sc_w)
  DevBuf w, w_wino, w_split, w_isplit, bias, lut, pre_scale, pre_shift;  // w_isplit: hi/lo halves for conv_igemm_split.hip  // w_wino: Winograd-transformed weights (3x3 s1 layers)
                                                               // w_split: fp16 hi/lo halves (conv_split.hip)
  WeightSets sets{};       // what pack_conv built (sets.wino: eligible for w_wino, built on first use)
  int cout_pad = 0;        // weight rows / bias padded to whole 64-wide tiles
  float pre_smax = 1.f, pre_bmax = 0.f;  // bound of the BN + ReLU prologue: |x_act| <= pre_smax max|x| + pre_bmax (ConvArgs::amax_a / amax_b)
  int se = 0;              // the input is gated by the squeeze-excitation vector of this block (1x1 projections)
  int run_mode = 0;        // stem with K ordered (kh, [kw x cin run]) over an UNPADDED 6-channel input, see pack_conv
  // fp16 plan: cin rounded to 8, K to 64; packed halves, LUT per 8-half chunk, prologue in halves
  int cin16 = 0, Kpad16 = 0;
  DevBuf w16, lut16, pre_scale16, pre_shift16;
  DevBuf w_stem7;          // 7x7 stems followed by the max-pool: weights packed for conv_stem7.hip (fp32 or fp16 plan)
};

// one timed stretch of conv launches: a single launch (per-layer table, HP_PROFILE_LAYERS) or a run of
// consecutive conv launches (default: an event pair per launch costs 3 % of a refiner step)
struct EventPair { hipEvent_t e0 = nullptr, e1 = nullptr; double flops = 0.0, mfma_flops = 0.0; int conv = -1; int n = 0; };

// MBConv pieces (EfficientNet): depthwise conv + BN + swish, squeeze-excitation
struct DwLayer {
  std::string wname, bn;
  int C, k, stride, pad, H, W, Ho, Wo, in_buf, out_buf;
  DevBuf w, bias;
};
struct SeLayer {
  std::string prefix;  // "<block>._se_reduce" / "._se_expand"
  int C, Cse, HW, in_buf;
  DevBuf w1, b1, w2, b2;
};

enum OpKind { OP_CONV, OP_MAXPOOL, OP_HEAD, OP_DW, OP_SE, OP_RESIZE /* nearest to (Ho, Wo); C = stride mode flag in conv */ };
struct Op { OpKind kind; int conv = -1; int in_buf = -1, out_buf = -1; int H = 0, W = 0, C = 0, Ho = 0, Wo = 0; };

}  // namespace

struct Net {
  int arch, n_inputs, c_pad, h, w;
  bool finalized = false;
  int precision = HP_PRECISION_F32;
  DevBuf x16;  // fp16 plan: the network input converted to fp16 NHWC [max_batch][h][w][cin16 of the stem]
  int max_batch = 0;
  int device = -1;  // the HIP device that was current in hp_net_create: where the weights and the arena live
  std::map<std::string, std::vector<float>> params;
  std::vector<std::unique_ptr<ConvLayer>> convs;
  std::vector<std::unique_ptr<DwLayer>> dws;
  std::vector<std::unique_ptr<SeLayer>> ses;
  DevBuf se_pooled, se_gate, se_partial, se_sq;  // [max_batch][max expanded channels] (+ strip partial sums)
  int se_max_c = 0;
  float bn_eps = 1e-5f;       // nn.BatchNorm2d default (ResNets); 1e-3 for EfficientNet
  int n_features = 512;
  std::vector<Op> ops;
  std::vector<size_t> buf_floats_per_sample;  // arena slot sizes
  std::vector<DevBuf> bufs;
  DevBuf fc_w, fc_b, pose_w, pose_b, logit_w, logit_b;
  DevBuf head_ws;  // fc path of the head: 2 x [max_batch][512] floats
  float* pooled_out = nullptr;  // hp_net_set_pooled_out: where a forward also leaves the fc's input (head training)
  int pose_dim = 0, n_logits = 0;
  int feat_H = 0, feat_W = 0;
  struct FeatureMap { int buf, H, W, C; };
  std::vector<FeatureMap> feature_maps;  // detector backbone: the FPN levels ('0', '1', '2', '3', 'pool'), arena slots
  double flops_per_sample = 0.0;
  bool profiling = false;
  std::vector<EventPair> ev_pending, ev_pool;  // conv-launch event pairs (profiling only)
  // per-network switches (no process-wide state on the launch path)
  int algo = -1;               // HP_CONV_ALGO_*; -1 = follow the process-wide default (hp_conv_select_algo / environment)
  bool tail_split = true;      // K-slicing of tail tiles (off while a second lane shares the GPU)
  bool act_scale = true;       // dynamic power-of-two activation scale of the split-fp16 kernels (hp_net_set_act_scale)
  // non-finite guard of the split-fp16 kernels: a host-visible word the epilogues set (hipHostMalloc, coherent)
  unsigned* h_status = nullptr;  // host address
  unsigned* d_status = nullptr;  // the same word as the device sees it
  bool exact_only = false;       // sticky after the guard fired: exact-fp32 kernels only
  // dynamic range of the split-fp16 kernels (ConvArgs::amax_in / amax_out): one word per op, zeroed at the start of a forward
  DevBuf amax;
  // layer-level tests (hp_net_set_taps / hp_net_op_info): per op, where to copy its output and what the last forward launched
  std::vector<void*> taps;       // empty = no taps; else one entry per op (nullptr = not tapped)
  std::vector<int> op_path;      // HP_PATH_* per op
  std::vector<char> op_mat;      // the op's output map was written
  ~Net() { if (h_status) (void)hipHostFree(h_status); }
};

namespace {

const std::vector<float>* find(const Net& n, const std::string& k) {
  auto it = n.params.find(k);
  return it == n.params.end() ? nullptr : &it->second;
}

int need(const Net& n, const std::string& k, size_t numel, const std::vector<float>** out) {
  const std::vector<float>* v = find(n, k);
  if (!v) return fail(HP_ERR_STATE, "missing parameter '" + k + "'");
  if (v->size() != numel)
    return fail(HP_ERR_ARG, "parameter '" + k + "' has " + std::to_string(v->size()) + " elements, expected " + std::to_string(numel));
  *out = v;
  return HP_OK;
}

// scale = gamma / sqrt(var + eps), shift = beta - mean * scale
int bn_affine(const Net& n, const std::string& p, int c, std::vector<float>& scale, std::vector<float>& shift) {
  const std::vector<float>*g, *b, *m, *v;
  int rc;
  if ((rc = need(n, p + ".weight", c, &g))) return rc;
  if ((rc = need(n, p + ".bias", c, &b))) return rc;
  if ((rc = need(n, p + ".running_mean", c, &m))) return rc;
  if ((rc = need(n, p + ".running_var", c, &v))) return rc;
  scale.resize(c); shift.resize(c);
  for (int i = 0; i < c; ++i) {
    const float s = (*g)[i] / std::sqrt((*v)[i] + n.bn_eps);
    scale[i] = s;
    shift[i] = (*b)[i] - (*m)[i] * s;
  }
  return HP_OK;
}

int add_conv(Net& n, const std::string& wname, const std::string& bn_after, const std::string& bn_before,
             int cin_real, int cout, int k, int stride, int pad, int relu, int H, int W, int in_buf,
             int out_buf, int res_buf, int Ho = -1, int Wo = -1) {
  auto L = std::make_unique<ConvLayer>();
  L->wname = wname; L->bn_after = bn_after; L->bn_before = bn_before;
  L->cin_real = cin_real; L->cin = (cin_real + 3) / 4 * 4; L->cout = cout; L->kh = L->kw = k;
  L->stride = stride; L->pad = pad; L->relu = relu; L->H = H; L->W = W;
  L->Ho = Ho > 0 ? Ho : (H + 2 * pad - k) / stride + 1;  // explicit for asymmetric "same" padding
  L->Wo = Wo > 0 ? Wo : (W + 2 * pad - k) / stride + 1;
  L->Kpad = (k * k * L->cin + 31) / 32 * 32;
  L->cout_pad = (cout + 63) / 64 * 64;
  L->in_buf = in_buf; L->out_buf = out_buf; L->res_buf = res_buf;
  n.flops_per_sample += 2.0 * L->Ho * L->Wo * cout * k * k * cin_real;
  Op op; op.kind = OP_CONV; op.conv = (int)n.convs.size();
  n.convs.push_back(std::move(L));
  n.ops.push_back(op);
  return n.ops.back().conv;
}

void want(Net& n, int slot, size_t floats) {
  if ((int)n.buf_floats_per_sample.size() <= slot) n.buf_floats_per_sample.resize(slot + 1, 0);
  if (n.buf_floats_per_sample[slot] < floats) n.buf_floats_per_sample[slot] = floats;
}

// the two memory-bound ops of an MBConv block (EfficientNet plan; caller-described graphs: hp_net_add_dwconv / hp_net_add_se)
void add_dw(Net& n, const std::string& wname, const std::string& bn, int C, int k, int stride, int pad, int H, int W, int Ho, int Wo,
            int in_buf, int out_buf) {
  auto D = std::make_unique<DwLayer>();
  D->wname = wname; D->bn = bn;
  D->C = C; D->k = k; D->stride = stride; D->pad = pad; D->H = H; D->W = W; D->Ho = Ho; D->Wo = Wo;
  D->in_buf = in_buf; D->out_buf = out_buf;
  n.flops_per_sample += 2.0 * Ho * Wo * C * k * k;
  Op od; od.kind = OP_DW; od.conv = (int)n.dws.size();
  n.dws.push_back(std::move(D)); n.ops.push_back(od);
}

void add_se(Net& n, const std::string& prefix, int C, int Cse, int HW, int in_buf) {
  auto S = std::make_unique<SeLayer>();
  S->prefix = prefix; S->C = C; S->Cse = Cse; S->HW = HW; S->in_buf = in_buf;
  n.se_max_c = std::max(n.se_max_c, C);
  n.flops_per_sample += 2.0 * 2.0 * C * Cse;
  Op os; os.kind = OP_SE; os.conv = (int)n.ses.size();
  n.ses.push_back(std::move(S)); n.ops.push_back(os);
}

// Build the op list.  Arena slots: 0 = stem output, then a rotating set of 4.
int build_graph(Net& n) {
  n.convs.clear(); n.ops.clear(); n.buf_floats_per_sample.clear(); n.flops_per_sample = 0.0;
  const bool vanilla = n.arch == HP_ARCH_VANILLA_RESNET34;
  const int* layers = n.arch == HP_ARCH_WIDE_RESNET18 ? kLayers18 : kLayers34;
  const std::string bb = "backbone.";
  const int k1 = vanilla ? 7 : 5;
  int c = add_conv(n, bb + "conv1.weight", bb + "bn1", "", n.n_inputs, 64, k1, 2, k1 / 2, 1, n.h, n.w, -1, 0, -1);
  if (!vanilla && n.n_inputs == 6 && n.w % 2 == 0) {
    // CosyPose stem (5x5, stride 2, 6 channels): the 5 taps x 6 channels of a filter row are 30
    // CONTIGUOUS floats of an unpadded NHWC input, so K = 5 rows x 32 = 160 instead of 25 taps x 8
    // padded channels = 200 (-> 224): 29 % less matrix work in the largest launch of a forward.
    // 16-B chunk alignment holds because a pixel is 24 B and tap offsets are even; a chunk covers
    // taps {0}, {0,1}, {1}, {2}, {2,3}, {3}, {4}, {4,pad} and the taps that fall outside the image
    // at the left / right border ({0,1} / {4}) cover whole chunks, so validity stays per chunk.
    ConvLayer& S = *n.convs[c];
    S.run_mode = 1; S.cin = 6; S.Kpad = 5 * 32;
    n.c_pad = 6;
  }
  int H = n.convs[c]->Ho, W = n.convs[c]->Wo;
  want(n, 0, (size_t)H * W * 64);
  Op mp; mp.kind = OP_MAXPOOL; mp.in_buf = 0; mp.out_buf = 1; mp.H = H; mp.W = W; mp.C = 64;
  mp.Ho = (H + 2 - 3) / 2 + 1; mp.Wo = (W + 2 - 3) / 2 + 1;
  n.ops.push_back(mp);
  H = mp.Ho; W = mp.Wo;
  want(n, 1, (size_t)H * W * 64);
  int cur = 1, inpl = 64;
  auto next_free = [&](std::initializer_list<int> used) {
    for (int s = 1; s <= 4; ++s) {
      bool u = false;
      for (int x : used) u |= (x == s);
      if (!u) return s;
    }
    return -1;
  };
  for (int li = 0; li < 4; ++li) {
    const int planes = kPlanes[li];
    for (int b = 0; b < layers[li]; ++b) {
      const int stride = (b == 0 && li > 0) ? 2 : 1;
      const bool ds = stride != 1 || inpl != planes;
      const std::string p = bb + "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
      const int t = next_free({cur});
      const int d = ds ? next_free({cur, t}) : -1;
      const int o = next_free({cur, t, ds ? d : cur});
      want(n, t, (size_t)Ho * Wo * planes);
      want(n, o, (size_t)Ho * Wo * planes);
      if (ds) want(n, d, (size_t)Ho * Wo * planes);
      if (vanilla) {
        add_conv(n, p + ".conv1.weight", p + ".bn1", "", inpl, planes, 3, stride, 1, 1, H, W, cur, t, -1);
        if (ds) add_conv(n, p + ".downsample.0.weight", p + ".downsample.1", "", inpl, planes, 1, stride, 0, 0, H, W, cur, d, -1);
        add_conv(n, p + ".conv2.weight", p + ".bn2", "", planes, planes, 3, 1, 1, 1, Ho, Wo, t, o, ds ? d : cur);
      } else {
        add_conv(n, p + ".conv1.weight", p + ".bn2", p + ".bn1", inpl, planes, 3, stride, 1, 1, H, W, cur, t, -1);
        // (the module computes the shortcut first: same values; behind conv1 it can ride in conv1's launch, forward_chunk)
        if (ds) add_conv(n, p + ".downsample.weight", "", p + ".bn1", inpl, planes, 1, stride, 0, 0, H, W, cur, d, -1);
        add_conv(n, p + ".conv2.weight", "", "", planes, planes, 3, 1, 1, 0, Ho, Wo, t, o, ds ? d : cur);
      }
      cur = o; inpl = planes; H = Ho; W = Wo;
    }
  }
  Op hd; hd.kind = OP_HEAD; hd.in_buf = cur; hd.H = H; hd.W = W; hd.C = 512;
  n.ops.push_back(hd);
  n.feat_H = H; n.feat_W = W;
  if (vanilla) n.flops_per_sample += 2.0 * 512 * 512;
  return HP_OK;
}

// ---- EfficientNet-b3 (CP/models/efficientnet.py; width 1.2, depth 1.4, static "same" padding
//      computed for image_size 300: efficientnet_utils.py:183-212,241-256,339-367) -----------------
int eff_round_filters(int f) {  // round_filters: width 1.2, divisor 8
  const double x = f * 1.2;
  int nf = std::max(8, (int)(x + 4) / 8 * 8);
  if (nf < 0.9 * x) nf += 8;
  return nf;
}

void eff_same_pad(int k, int stride, int* lo, int* total) {  // padding fixed for a 300-pixel image
  const int o = (300 + stride - 1) / stride;
  *total = std::max((o - 1) * stride + k - 300, 0);
  *lo = *total / 2;
}

int build_graph_efficientnet(Net& n) {
  n.convs.clear(); n.dws.clear(); n.ses.clear(); n.ops.clear(); n.buf_floats_per_sample.clear();
  n.flops_per_sample = 0.0; n.bn_eps = 1e-3f; n.se_max_c = 0;
  const std::string bb = "backbone.";
  static const int base[7][6] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80},
                                 {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192}, {1, 3, 1, 6, 192, 320}};
  // arena slots: 0 / 1 = block input / output (ping-pong), 2 = expanded, 3 = depthwise output
  int lo, tot;
  eff_same_pad(3, 2, &lo, &tot);
  int H = (n.h + tot - 3) / 2 + 1, W = (n.w + tot - 3) / 2 + 1;
  const int stem = eff_round_filters(32);
  add_conv(n, bb + "_conv_stem.weight", bb + "_bn0", "", n.n_inputs, stem, 3, 2, lo, HP_ACT_SWISH, n.h, n.w, -1, 0, -1, H, W);
  want(n, 0, (size_t)H * W * stem);
  int cur = 0, bi = 0, inpl = stem;
  for (const auto& st : base) {
    const int reps = (int)std::ceil(1.4 * st[0]), k = st[1], e = st[3];
    const int out_f = eff_round_filters(st[5]);
    for (int j = 0; j < reps; ++j, ++bi) {
      const int stride = j == 0 ? st[2] : 1;
      const int cin = j == 0 ? eff_round_filters(st[4]) : out_f;
      if (cin != inpl) return fail(HP_ERR_STATE, "efficientnet plan: channel mismatch");
      const int mid = cin * e, cse = std::max(1, (int)(cin * 0.25));
      const std::string p = bb + "_blocks." + std::to_string(bi);
      int src = cur;
      if (e != 1) {
        add_conv(n, p + "._expand_conv.weight", p + "._bn0", "", cin, mid, 1, 1, 0, HP_ACT_SWISH, H, W, cur, 2, -1);
        want(n, 2, (size_t)H * W * mid);
        src = 2;
      }
      eff_same_pad(k, stride, &lo, &tot);
      const int Ho = (H + tot - k) / stride + 1, Wo = (W + tot - k) / stride + 1;
      add_dw(n, p + "._depthwise_conv.weight", p + "._bn1", mid, k, stride, lo, H, W, Ho, Wo, src, 3);
      want(n, 3, (size_t)Ho * Wo * mid);
      add_se(n, p, mid, cse, Ho * Wo, 3);
      const bool skip = stride == 1 && cin == out_f;
      const int dst = 1 - cur;
      const int c = add_conv(n, p + "._project_conv.weight", p + "._bn2", "", mid, out_f, 1, 1, 0, HP_ACT_NONE, Ho, Wo, 3, dst,
                             skip ? cur : -1);
      n.convs[c]->se = 1;
      want(n, dst, (size_t)Ho * Wo * out_f);
      cur = dst; H = Ho; W = Wo; inpl = out_f;
    }
  }
  const int head = eff_round_filters(1280);
  add_conv(n, bb + "_conv_head.weight", bb + "_bn1", "", inpl, head, 1, 1, 0, HP_ACT_SWISH, H, W, cur, 2, -1);
  want(n, 2, (size_t)H * W * head);
  Op hd; hd.kind = OP_HEAD; hd.in_buf = 2; hd.H = H; hd.W = W; hd.C = head;
  n.ops.push_back(hd);
  n.feat_H = H; n.feat_W = W; n.n_features = head;
  return HP_OK;
}

// ---- ResNet-50 + FPN, the backbone of the Mask-RCNN detector (MP/models/mask_rcnn.py:22-42:
//      torchvision resnet_fpn_backbone("resnet50"): models/resnet.py Bottleneck (stride on the 3x3 conv), BatchNorm2d in
//      eval mode, ops/feature_pyramid_network.py with LastLevelMaxPool).  State-dict keys as the reference's
//      DetectorMaskRCNN registers them: backbone.body.*, backbone.fpn.inner_blocks.N.0.*, backbone.fpn.layer_blocks.N.0.*.
//      Arena slots: 0 stem, 1 pooled stem, 2..4 block scratch (t1, t2, downsample), 5/6 ping-pong block outputs,
//      7..10 = C2..C5, 11..14 lateral sums, 15 upsampled, 16..19 = P2..P5, 20 = pool.
int build_graph_r50fpn(Net& n) {
  n.convs.clear(); n.ops.clear(); n.buf_floats_per_sample.clear(); n.flops_per_sample = 0.0; n.feature_maps.clear();
  const std::string bb = "backbone.body.";
  int c = add_conv(n, bb + "conv1.weight", bb + "bn1", "", n.n_inputs, 64, 7, 2, 3, 1, n.h, n.w, -1, 0, -1);
  int H = n.convs[c]->Ho, W = n.convs[c]->Wo;
  want(n, 0, (size_t)H * W * 64);
  Op mp; mp.kind = OP_MAXPOOL; mp.in_buf = 0; mp.out_buf = 1; mp.H = H; mp.W = W; mp.C = 64;
  mp.Ho = (H + 2 - 3) / 2 + 1; mp.Wo = (W + 2 - 3) / 2 + 1;
  n.ops.push_back(mp);
  H = mp.Ho; W = mp.Wo;
  want(n, 1, (size_t)H * W * 64);
  int cur = 1, inpl = 64;
  int level_buf[4], level_H[4], level_W[4];
  for (int li = 0; li < 4; ++li) {
    const int planes = kPlanes[li], outc = planes * 4;
    for (int b = 0; b < kLayers34[li]; ++b) {  // ResNet-50 has the [3, 4, 6, 3] layout of ResNet-34
      const int stride = (b == 0 && li > 0) ? 2 : 1;
      const bool ds = b == 0;
      const std::string p = bb + "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
      const bool last = b == kLayers34[li] - 1;
      const int o = last ? 7 + li : (cur == 5 ? 6 : 5);
      want(n, 2, (size_t)H * W * planes);
      want(n, 3, (size_t)Ho * Wo * planes);
      want(n, o, (size_t)Ho * Wo * outc);
      add_conv(n, p + ".conv1.weight", p + ".bn1", "", inpl, planes, 1, 1, 0, 1, H, W, cur, 2, -1);
      add_conv(n, p + ".conv2.weight", p + ".bn2", "", planes, planes, 3, stride, 1, 1, H, W, 2, 3, -1);
      int res = cur;
      if (ds) {
        want(n, 4, (size_t)Ho * Wo * outc);
        add_conv(n, p + ".downsample.0.weight", p + ".downsample.1", "", inpl, outc, 1, stride, 0, 0, H, W, cur, 4, -1);
        res = 4;
      }
      add_conv(n, p + ".conv3.weight", p + ".bn3", "", planes, outc, 1, 1, 0, 1, Ho, Wo, 3, o, res);
      cur = o; inpl = outc; H = Ho; W = Wo;
    }
    level_buf[li] = cur; level_H[li] = H; level_W[li] = W;
  }
  // FPN (ops/feature_pyramid_network.py: FeaturePyramidNetwork.forward)
  const std::string fp = "backbone.fpn.";
  int last_inner = -1;
  for (int li = 3; li >= 0; --li) {
    const int Hl = level_H[li], Wl = level_W[li], cin = kPlanes[li] * 4;
    const std::string ib = fp + "inner_blocks." + std::to_string(li) + ".0";
    int res = -1;
    if (last_inner >= 0) {  // top-down: nearest upsampling of the coarser lateral sum to this level's size
      Op up; up.kind = OP_RESIZE; up.in_buf = last_inner; up.out_buf = 15; up.H = level_H[li + 1]; up.W = level_W[li + 1]; up.C = 256;
      up.Ho = Hl; up.Wo = Wl; up.conv = 0;
      n.ops.push_back(up);
      want(n, 15, (size_t)Hl * Wl * 256);
      res = 15;
    }
    const int inner = 11 + li;
    want(n, inner, (size_t)Hl * Wl * 256);
    int ci = add_conv(n, ib + ".weight", "", "", cin, 256, 1, 1, 0, 0, Hl, Wl, level_buf[li], inner, res);
    n.convs[ci]->bias_name = ib + ".bias";
    const std::string lb = fp + "layer_blocks." + std::to_string(li) + ".0";
    want(n, 16 + li, (size_t)Hl * Wl * 256);
    int co = add_conv(n, lb + ".weight", "", "", 256, 256, 3, 1, 1, 0, Hl, Wl, inner, 16 + li, -1);
    n.convs[co]->bias_name = lb + ".bias";
    last_inner = inner;
  }
  // LastLevelMaxPool: max_pool2d(P5, 1, 2, 0)
  Op sp; sp.kind = OP_RESIZE; sp.in_buf = 19; sp.out_buf = 20; sp.H = level_H[3]; sp.W = level_W[3]; sp.C = 256;
  sp.Ho = (level_H[3] - 1) / 2 + 1; sp.Wo = (level_W[3] - 1) / 2 + 1; sp.conv = 1;
  n.ops.push_back(sp);
  want(n, 20, (size_t)sp.Ho * sp.Wo * 256);
  for (int li = 0; li < 4; ++li) n.feature_maps.push_back({16 + li, level_H[li], level_W[li], 256});
  n.feature_maps.push_back({20, sp.Ho, sp.Wo, 256});
  // RPN head on every level, shared weights (torchvision models/detection/rpn.py: RPNHead: conv 3x3 + ReLU, then
  // cls_logits 1x1 -> 3 anchors and bbox_pred 1x1 -> 12 deltas): maps 5..9 = objectness [h][w][4] (channel 3 is padding),
  // maps 10..14 = deltas [h][w][12].  Slot 21 = the shared 3x3 output, 22.. = per-level outputs.
  const std::string rp = "rpn.head.";
  for (int l = 0; l < 5; ++l) {
    const Net::FeatureMap fm = n.feature_maps[l];
    want(n, 21, (size_t)fm.H * fm.W * 256);
    int c0 = add_conv(n, rp + "conv.0.0.weight", "", "", 256, 256, 3, 1, 1, 1, fm.H, fm.W, fm.buf, 21, -1);
    n.convs[c0]->bias_name = rp + "conv.0.0.bias";
    want(n, 22 + l, (size_t)fm.H * fm.W * 4);
    int c1 = add_conv(n, rp + "cls_logits.weight", "", "", 256, 4, 1, 1, 0, 0, fm.H, fm.W, 21, 22 + l, -1);
    n.convs[c1]->bias_name = rp + "cls_logits.bias"; n.convs[c1]->cout_real = 3;
    want(n, 27 + l, (size_t)fm.H * fm.W * 12);
    int c2 = add_conv(n, rp + "bbox_pred.weight", "", "", 256, 12, 1, 1, 0, 0, fm.H, fm.W, 21, 27 + l, -1);
    n.convs[c2]->bias_name = rp + "bbox_pred.bias";
  }
  for (int l = 0; l < 5; ++l) n.feature_maps.push_back({22 + l, n.feature_maps[l].H, n.feature_maps[l].W, 4});
  for (int l = 0; l < 5; ++l) n.feature_maps.push_back({27 + l, n.feature_maps[l].H, n.feature_maps[l].W, 12});
  n.feat_H = sp.Ho; n.feat_W = sp.Wo; n.n_features = 256;
  return HP_OK;
}

// ---- Choosing a conv's kernel: one description of a conv site, one statement of the weight sets a layer
//      gets, one ladder.  The networks (forward_chunk) and the single-layer entry (hp_conv2d_nhwc) both go through them. ----
struct ConvSite {
  // the layer
  int H = 0, W = 0, Cin = 0, cin_real = 0, Ho = 0, Wo = 0, Cout = 0, kh = 0, kw = 0, stride = 1, pad = 0;
  int act = HP_ACT_NONE;
  bool se_gated = false;  // the input is multiplied by a per-image gate (pre_scale alone)
  bool prologue = false;  // BN + ReLU on the input (pre_scale and pre_shift)
  bool residual = false, bias = false;
  int cout_pad = 0, Kpad = 0, run_mode = 0;
  // the two rules of the single-layer entry, which transforms a weight set per call ("where the entries differ")
  bool isplit_beside_split = false;  // the igemm-split set exists for a layer that has the 3x3 split set too
  bool wino_classic_only = false;    // Winograd for unpadded, non-swish, ungated layers only
  // the weight sets that exist, the algorithm, the batch
  bool has_split = false, has_isplit = false, has_wino = false, has_stem7 = false;
  int algo = HP_CONV_ALGO_AUTO, batch = 1;
  // what the neighbours allow
  bool pool_follows = false;      // a max-pool op reads this map next (the fused stems write the pooled map instead)
  bool dw_se_follow = false;      // a depthwise conv of this map and its squeeze-excitation follow, wired for the fused front
  int dw_k = 0, dw_stride = 0, dw_Ho = 0, dw_Wo = 0;
  bool shortcut_follows = false;  // op o+1 is the block's 1x1 / stride-2 shortcut and may ride (shortcut_may_ride)
  bool per_launch = false, sync_ops = false, no_sc_fusion = false;  // diagnostics that keep every launch apart
};

// the site as the *_applicable / *_launchable predicates take it; they test the pointers and never read through them
ConvArgs site_args(const ConvSite& s) {
  static const float set = 0.f;
  ConvArgs a{};
  a.H = s.H; a.W = s.W; a.Cin = s.Cin; a.Ho = s.Ho; a.Wo = s.Wo; a.Cout = s.Cout; a.stride = s.stride; a.pad = s.pad;
  a.Kpad = s.Kpad; a.ktiles = s.Kpad / 32; a.relu = s.act; a.M = (int64_t)s.batch * s.Ho * s.Wo;
  a.pre_scale = s.prologue || s.se_gated ? &set : nullptr; a.pre_shift = s.prologue ? &set : nullptr;
  a.residual = s.residual ? &set : nullptr; a.bias = s.bias ? &set : nullptr;
  return a;
}

// Which weight sets a layer gets (batch independent): pack_conv builds them, ensure_wino_weights builds `wino` on first use,
// hp_conv2d_nhwc transforms the one its launch needs per call.
WeightSets conv_weight_sets(const ConvSite& s) {
  const ConvArgs a = site_args(s);
  const bool plain_act = s.act != HP_ACT_SWISH && !s.se_gated;
  const bool classic = plain_act && s.cout_pad == s.Cout && s.Kpad == s.kh * s.kw * s.Cin;  // what the 3x3 kernels support
  WeightSets r{};
  r.split = plain_act && conv_split_applicable(a, s.kh, s.kw);  // fp16 hi / lo halves for conv_split.hip
  r.isplit = (!r.split || s.isplit_beside_split) && s.Kpad % 32 == 0;  // ... for conv_igemm_split.hip: every other layer,
                                                                        // swish layers and SE-gated projections included
  r.wino = conv_wino_applicable(a, s.kh, s.kw) && (classic || !s.wino_classic_only);
  r.stem7 = conv_stem7_applicable(s.kh, s.kw, s.stride, s.pad, s.Cin, s.Cout, s.act, 0) && !s.run_mode && !s.prologue;
  // a 1x1 / stride-2 / pad-0 shortcut whose 3x3 / stride-2 / pad-1 twin the persistent stride-2 kernel would take
  ConvArgs twin = a;
  twin.pad = 1;
  r.shortcut = s.kh == 1 && s.kw == 1 && s.stride == 2 && s.pad == 0 && !s.residual && conv_pp_s2_applicable(twin, 3, 3) &&
               s.cout_pad == s.Cout && s.cin_real == s.Cin && plain_act;
  return r;
}

enum WeightSet { W_PACKED, W_SPLIT, W_ISPLIT, W_WINO, W_STEM7 };
struct ConvChoice {
  int path = HP_PATH_GENERIC;
  WeightSet w = W_PACKED;        // the set ConvArgs::w points at
  int variant = 0;               // 128x128 tiles, or 128x64
  bool pool_fused = false, front_fused = false, shortcut_rides = false;  // what the launch absorbs
  bool materialised = true;      // the output map is written
  bool tracks_amax = true;       // the launch goes through the shared epilogue (ConvArgs::amax_out)
  bool status = false;           // split-fp16 arithmetic: the launch gets the non-finite guard word
  // FLOPs the matrix cores execute (padded tiles / K included).  Split-fp16 launches: three fp16 MFMAs per product, and an
  // fp16 MFMA FLOP occupies the pipe for 1/16 of an fp32 one, so it counts 1/16: mfma_flops / time / fp32 peak stays "how
  // busy is the pipe".  sc_mfma_flops: the riding shortcut's share (accounted as a launch of its own).
  double mfma_flops = 0.0, sc_mfma_flops = 0.0;
};

// The ladder.  Pure: launches nothing, reads no Net.
ConvChoice choose_conv(const ConvSite& s) {
  const ConvArgs a = site_args(s);
  const bool split_algo = conv_algo_uses_split(s.algo);
  const bool wino_algo = s.algo == HP_CONV_ALGO_AUTO || s.algo == HP_CONV_ALGO_WINOGRAD_1WAVE || s.algo == HP_CONV_ALGO_WINOGRAD;
  ConvChoice c;
  c.variant = s.cout_pad % 128 == 0 ? 0 : 1;
  if (s.dw_se_follow && s.has_isplit && s.kh == 1 && s.act == HP_ACT_SWISH && !s.se_gated && !s.residual && !s.prologue && s.bias &&
      split_algo && mbconv_front_applicable(s.Cin, s.Kpad, s.Cout, s.dw_k, s.dw_stride)) {
    // MBConv front: expansion + depthwise (+ SE pooling sums) in one launch, the expanded tensor stays on the CU
    c.path = HP_PATH_MBCONV_FRONT; c.w = W_ISPLIT; c.front_fused = true; c.status = true;
    const int th = s.dw_stride == 1 ? 8 : 4, tw = s.dw_stride == 1 ? 16 : 8;
    const int rows = (((th - 1) * s.dw_stride + s.dw_k) * ((tw - 1) * s.dw_stride + s.dw_k) + 31) / 32 * 32;
    c.mfma_flops = 2.0 * (double)s.batch * mbconv_front_tiles(s.dw_Ho, s.dw_Wo, s.dw_stride) * rows * ((s.Cout + 31) / 32 * 32) * s.Kpad * 3.0 / 16.0;
  } else if (split_algo && s.has_stem7 && s.pool_follows) {
    // MegaPose stem + ReLU + max-pool in one launch, the input region of a pooled tile staged once per channel slab
    c.path = HP_PATH_STEM7_POOL; c.w = W_STEM7; c.pool_fused = true; c.status = true;
    const int sc = s.Cin % 8 == 0 ? 8 : 4, ks = (7 * sc + 15) / 16;
    c.mfma_flops = 3.0 / 16.0 * 2.0 * (double)a.M * (256.0 / 192.0) * s.Cout * (s.Cin / sc) * 7.0 * ks * 16.0;
  } else if (split_algo && s.has_split && conv_split_launchable(a)) {
    // A down-sampling block's 1x1 / stride-2 shortcut runs as extra work items of the block's 3x3 / stride-2 launch
    // (conv3x3s2_pp, ConvArgs::sc_w): as a launch of its own it sits on a floor of 20 - 30 us whatever the kernel
    c.shortcut_rides = s.shortcut_follows && !s.no_sc_fusion && !s.per_launch && !s.sync_ops;
    c.path = c.shortcut_rides ? HP_PATH_SPLIT3X3_SHORTCUT : HP_PATH_SPLIT3X3; c.w = W_SPLIT; c.status = true;
    if (c.shortcut_rides) c.sc_mfma_flops = 3.0 * 2.0 * (double)((a.M + 255) / 256 * 256) * s.Cout * s.Cin / 16.0;
    // whole 256- / 512-row tiles; 256-row tiles on the ping-pong kernel
    const int64_t bm = (s.Cout % 128 == 0 || (s.stride == 1 && conv_pp_split_applicable(a, s.kh, s.kw))) ? 256 : 512;
    c.mfma_flops = 3.0 * 2.0 * (double)((a.M + bm - 1) / bm * bm) * s.Cout * s.Kpad / 16.0;
  } else if (wino_algo && s.has_wino && conv_wino_launchable(a)) {
    // exact fp32: 16 multiplies per 2x2 output tile, cin and cout
    c.path = HP_PATH_WINOGRAD; c.w = W_WINO; c.tracks_amax = false;
    c.mfma_flops = 2.0 * 16.0 * (double)s.batch * ((s.Ho + 1) / 2) * ((s.Wo + 1) / 2) * s.Cin * s.Cout;
  } else {
    c.mfma_flops = 2.0 * (double)((a.M + 127) / 128 * 128) * s.cout_pad * s.Kpad;  // M x Cout x Kpad
    if (split_algo && s.has_isplit && conv_igemm_split_launchable(a)) {
      c.path = HP_PATH_IGEMM_SPLIT; c.w = W_ISPLIT; c.status = true;
      if (s.pool_follows && conv_igemm_split_pool_launchable(a, s.cout_pad)) {
        // stem + ReLU + 3x3/s2 max-pool in one launch: the conv map is never written
        c.pool_fused = true;
        if (conv_stem_split_applicable(a, s.kh, s.kw, s.run_mode)) {
          c.path = HP_PATH_STEM_SPLIT_POOL;
          c.mfma_flops *= 256.0 / 192.0;  // 256 GEMM rows per 6 x 32 conv pixels (7 x 33 computed, the rest padding)
        } else {
          c.path = HP_PATH_IGEMM_SPLIT_POOL;
          c.mfma_flops *= 1.24;  // conv pixels under the tile borders are computed twice (7 x 17 per 6 x 16)
        }
      }
      c.mfma_flops *= 3.0 / 16.0;
    } else if (s.algo != HP_CONV_ALGO_IGEMM && s.act != HP_ACT_SWISH && !s.se_gated && conv_patch_applicable(a, s.kh, s.kw)) {
      c.path = HP_PATH_PATCH;
    }
  }
  if (c.pool_fused || c.front_fused) { c.materialised = false; c.tracks_amax = false; }
  return c;
}

// the layer part of a network conv's site (the sets that exist, algorithm, batch and neighbours are the forward's to add)
ConvSite layer_site(const ConvLayer& L) {
  ConvSite s;
  s.H = L.H; s.W = L.W; s.Cin = L.cin; s.cin_real = L.cin_real; s.Ho = L.Ho; s.Wo = L.Wo; s.Cout = L.cout; s.kh = L.kh; s.kw = L.kw;
  s.stride = L.stride; s.pad = L.pad; s.act = L.relu; s.se_gated = L.se != 0; s.prologue = !L.bn_before.empty() && !L.se;
  s.residual = L.res_buf >= 0; s.cout_pad = L.cout_pad; s.Kpad = L.Kpad; s.run_mode = L.run_mode;
  return s;
}

int pack_conv(Net& n, ConvLayer& L) {
  const std::vector<float>* w;
  const int rows = L.cout_real ? L.cout_real : L.cout;
  const size_t numel = (size_t)rows * L.cin_real * L.kh * L.kw;
  int rc = need(n, L.wname, numel, &w);
  if (rc) return rc;
  std::vector<float> scale, shift;
  if (!L.bn_after.empty() && (rc = bn_affine(n, L.bn_after, L.cout, scale, shift))) return rc;
  std::vector<float> packed((size_t)L.cout_pad * L.Kpad, 0.f);  // rows padded to whole 64-wide tiles
  const int run = (L.kw * L.cin + 3) / 4 * 4;  // run mode: floats per filter row (30 -> 32)
  for (int o = 0; o < rows; ++o) {
    const float s = scale.empty() ? 1.f : scale[o];
    for (int ci = 0; ci < L.cin_real; ++ci)
      for (int y = 0; y < L.kh; ++y)
        for (int x = 0; x < L.kw; ++x) {
          const size_t k = L.run_mode ? (size_t)y * run + (size_t)x * L.cin + ci : (size_t)(y * L.kw + x) * L.cin + ci;
          packed[(size_t)o * L.Kpad + k] = (*w)[(((size_t)o * L.cin_real + ci) * L.kh + y) * L.kw + x] * s;
        }
  }
  if ((rc = L.w.upload(packed.data(), packed.size() * 4))) return rc;
  const WeightSets sets = L.sets = conv_weight_sets(layer_site(L));
  // The Winograd weight set (exact-fp32 U = G g G^T) is LAZY: only eligibility is recorded here; ensure_wino_weights()
  // transforms it the first time a forward's algorithm can reach it (the guard's exact-fp32 fallback,
  // hp_net_set_conv_algo).  The default plan never touches it: hp_net_create used to spend 150 MB and 58 transform
  // launches per WideResNet-34 on kernels that lost to the direct split kernels.
  if (sets.split) {
    if ((rc = L.w_split.alloc(conv_split_weight_bytes(L.cout, L.cin)))) return rc;
    if ((rc = conv_split_transform_weights((const float*)L.w.p, L.w_split.p, L.cout, L.cin, L.Kpad, L.stride, nullptr))) return rc;
    HP_CHECK_HIP(hipStreamSynchronize(nullptr));
  } else if (sets.isplit) {
    if ((rc = L.w_isplit.alloc(conv_igemm_split_weight_bytes(L.cout_pad, L.Kpad)))) return rc;
    if ((rc = conv_igemm_split_transform_weights((const float*)L.w.p, L.w_isplit.p, L.cout_pad, L.Kpad, nullptr))) return rc;
    HP_CHECK_HIP(hipStreamSynchronize(nullptr));
  }
  if (sets.shortcut) {
    std::vector<float> w33((size_t)L.cout * 9 * L.cin, 0.f);  // [cout][(kh, kw)][cin], centre tap = the shortcut
    for (int o = 0; o < L.cout; ++o)
      for (int ci = 0; ci < L.cin; ++ci) w33[((size_t)o * 9 + 4) * L.cin + ci] = packed[(size_t)o * L.Kpad + ci];
    DevBuf tmp;
    if ((rc = tmp.upload(w33.data(), w33.size() * 4))) return rc;
    if ((rc = L.w_short.alloc(conv_split_weight_bytes(L.cout, L.cin)))) return rc;
    if ((rc = conv_split_transform_weights((const float*)tmp.p, L.w_short.p, L.cout, L.cin, 9 * L.cin, 2, nullptr))) return rc;
    HP_CHECK_HIP(hipStreamSynchronize(nullptr));
  }
  if (sets.stem7) {
    std::vector<float> wf(numel);
    for (int o = 0; o < L.cout; ++o) {
      const float sc = scale.empty() ? 1.f : scale[o];
      for (size_t i = 0; i < (size_t)L.cin_real * 49; ++i) wf[(size_t)o * L.cin_real * 49 + i] = (*w)[(size_t)o * L.cin_real * 49 + i] * sc;
    }
    std::vector<unsigned char> pk(conv_stem7_pack_weights(wf.data(), L.cin_real, L.cin, 0, nullptr));
    conv_stem7_pack_weights(wf.data(), L.cin_real, L.cin, 0, pk.data());
    if ((rc = L.w_stem7.upload(pk.data(), pk.size()))) return rc;
  }
  if (!L.bias_name.empty()) {  // the convolution's own bias (no BN on these layers, or added to its shift)
    const std::vector<float>* b;
    if ((rc = need(n, L.bias_name, rows, &b))) return rc;
    if (shift.empty()) shift.assign(L.cout, 0.f);
    for (int o = 0; o < rows; ++o) shift[o] += (*b)[o];
  }
  if (!shift.empty()) {
    shift.resize(L.cout_pad, 0.f);  // read by whole tiles
    if ((rc = L.bias.upload(shift.data(), shift.size() * 4))) return rc;
  }
  if (!L.bn_before.empty()) {
    std::vector<float> ps, pb;
    if ((rc = bn_affine(n, L.bn_before, L.cin_real, ps, pb))) return rc;
    ps.resize(L.cin, 0.f); pb.resize(L.cin, 0.f);
    L.pre_smax = 0.f; L.pre_bmax = 0.f;
    for (int c = 0; c < L.cin; ++c) { L.pre_smax = std::fmax(L.pre_smax, std::fabs(ps[c])); L.pre_bmax = std::fmax(L.pre_bmax, std::fabs(pb[c])); }
    if ((rc = L.pre_scale.upload(ps.data(), ps.size() * 4))) return rc;
    if ((rc = L.pre_shift.upload(pb.data(), pb.size() * 4))) return rc;
  }
  // + 16 padding entries: the kernel prefetches the entries of K-tiles t+1 and t+2
  std::vector<int4> lut(L.Kpad / 4 + 16, make_int4(0, -1, 0, 0));
  const int kreal = L.run_mode ? L.kh * run : L.kh * L.kw * L.cin;
  for (int q = 0; q < L.Kpad / 4; ++q) {
    const int k = 4 * q;
    if (k >= kreal) {
      lut[q] = make_int4(0, -1, 0, 0);
    } else if (L.run_mode) {
      // chunk j of filter row y starts at float 4j of the run; validity follows its FIRST tap
      const int y = k / run, j4 = k % run;
      lut[q] = make_int4(y * L.W * L.cin + j4, y, j4 / L.cin, 0);
    } else {
      const int seg = k / L.cin, ch = k % L.cin, y = seg / L.kw, x = seg % L.kw;
      lut[q] = make_int4((y * L.W + x) * L.cin + ch, y, x, ch);
    }
  }
  return L.lut.upload(lut.data(), lut.size() * sizeof(int4));
}

int pack_dw(Net& n, DwLayer& D) {
  const std::vector<float>* w;
  int rc = need(n, D.wname, (size_t)D.C * D.k * D.k, &w);  // [C][1][k][k]
  if (rc) return rc;
  std::vector<float> scale, shift;
  if ((rc = bn_affine(n, D.bn, D.C, scale, shift))) return rc;
  std::vector<float> packed((size_t)D.k * D.k * D.C);
  for (int c = 0; c < D.C; ++c)
    for (int t = 0; t < D.k * D.k; ++t) packed[(size_t)t * D.C + c] = (*w)[(size_t)c * D.k * D.k + t] * scale[c];
  if ((rc = D.w.upload(packed.data(), packed.size() * 4))) return rc;
  return D.bias.upload(shift.data(), shift.size() * 4);
}

int pack_se(Net& n, SeLayer& S) {
  const std::vector<float>* v;
  int rc;
  if ((rc = need(n, S.prefix + "._se_reduce.weight", (size_t)S.Cse * S.C, &v))) return rc;
  if ((rc = S.w1.upload(v->data(), v->size() * 4))) return rc;
  if ((rc = need(n, S.prefix + "._se_reduce.bias", S.Cse, &v))) return rc;
  if ((rc = S.b1.upload(v->data(), v->size() * 4))) return rc;
  if ((rc = need(n, S.prefix + "._se_expand.weight", (size_t)S.C * S.Cse, &v))) return rc;
  {  // [C][Cse] -> [Cse][C]: lanes over c read it coalesced
    std::vector<float> t((size_t)S.C * S.Cse);
    for (int c = 0; c < S.C; ++c)
      for (int j = 0; j < S.Cse; ++j) t[(size_t)j * S.C + c] = (*v)[(size_t)c * S.Cse + j];
    if ((rc = S.w2.upload(t.data(), t.size() * 4))) return rc;
  }
  if ((rc = need(n, S.prefix + "._se_expand.bias", S.C, &v))) return rc;
  return S.b2.upload(v->data(), v->size() * 4);
}

// fp16 plan: BN folded in fp32, then rounded once to fp16; K order (kh, kw, c) with c padded to 8
int pack_conv_f16(Net& n, ConvLayer& L) {
  const std::vector<float>* w;
  const size_t numel = (size_t)L.cout * L.cin_real * L.kh * L.kw;
  int rc = need(n, L.wname, numel, &w);
  if (rc) return rc;
  std::vector<float> scale, shift;
  if (!L.bn_after.empty() && (rc = bn_affine(n, L.bn_after, L.cout, scale, shift))) return rc;
  L.cin16 = (L.cin_real + 7) / 8 * 8;
  L.Kpad16 = (L.kh * L.kw * L.cin16 + 63) / 64 * 64;
  std::vector<_Float16> packed((size_t)L.cout * L.Kpad16, (_Float16)0.f);
  for (int o = 0; o < L.cout; ++o) {
    const float s = scale.empty() ? 1.f : scale[o];
    for (int ci = 0; ci < L.cin_real; ++ci)
      for (int y = 0; y < L.kh; ++y)
        for (int x = 0; x < L.kw; ++x)
          packed[(size_t)o * L.Kpad16 + (size_t)(y * L.kw + x) * L.cin16 + ci] =
              (_Float16)((*w)[(((size_t)o * L.cin_real + ci) * L.kh + y) * L.kw + x] * s);
  }
  if ((rc = L.w16.upload(packed.data(), packed.size() * 2))) return rc;
  if (conv_stem7_applicable(L.kh, L.kw, L.stride, L.pad, L.cin16, L.cout, L.relu, 1) && L.bn_before.empty()) {
    std::vector<float> wf(numel);
    for (int o = 0; o < L.cout; ++o) {
      const float sc = scale.empty() ? 1.f : scale[o];
      for (size_t i = 0; i < (size_t)L.cin_real * 49; ++i) wf[(size_t)o * L.cin_real * 49 + i] = (*w)[(size_t)o * L.cin_real * 49 + i] * sc;
    }
    std::vector<unsigned char> pk(conv_stem7_pack_weights(wf.data(), L.cin_real, L.cin16, 1, nullptr));
    conv_stem7_pack_weights(wf.data(), L.cin_real, L.cin16, 1, pk.data());
    if ((rc = L.w_stem7.upload(pk.data(), pk.size()))) return rc;
  }
  if (!shift.empty() && (rc = L.bias.upload(shift.data(), shift.size() * 4))) return rc;
  if (!L.bn_before.empty()) {
    std::vector<float> ps, pb;
    if ((rc = bn_affine(n, L.bn_before, L.cin_real, ps, pb))) return rc;
    std::vector<_Float16> hs(L.cin16, (_Float16)0.f), hb(L.cin16, (_Float16)0.f);
    for (int i = 0; i < L.cin_real; ++i) { hs[i] = (_Float16)ps[i]; hb[i] = (_Float16)pb[i]; }
    if ((rc = L.pre_scale16.upload(hs.data(), hs.size() * 2))) return rc;
    if ((rc = L.pre_shift16.upload(hb.data(), hb.size() * 2))) return rc;
  }
  std::vector<int4> lut(L.Kpad16 / 8, make_int4(0, -1, 0, 0));
  const int kreal = L.kh * L.kw * L.cin16;
  for (int q = 0; q < L.Kpad16 / 8; ++q) {
    const int k = 8 * q;
    if (k < kreal) {
      const int seg = k / L.cin16, ch = k % L.cin16, y = seg / L.kw, x = seg % L.kw;
      lut[q] = make_int4((y * L.W + x) * L.cin16 + ch, y, x, ch);
    }
  }
  return L.lut16.upload(lut.data(), lut.size() * sizeof(int4));
}

}  // namespace
}  // namespace hp

struct hp_net : hp::Net {};

using namespace hp;

extern "C" hp_net* hp_net_create(int arch, int n_inputs, int h, int w) {
  if (arch < 0 || arch > HP_ARCH_CUSTOM || n_inputs < 1 || h < (arch == HP_ARCH_CUSTOM ? 1 : 32) || w < (arch == HP_ARCH_CUSTOM ? 1 : 32)) {
    set_error("hp_net_create: bad architecture / input shape");
    return nullptr;
  }
  hp_net* n = new hp_net();
  n->arch = arch; n->n_inputs = n_inputs; n->c_pad = (n_inputs + 3) / 4 * 4; n->h = h; n->w = w;
  (void)hipGetDevice(&n->device);
  if (arch == HP_ARCH_CUSTOM) return n;  // the caller describes the graph: hp_net_add_conv / hp_net_add_output
  if ((arch == HP_ARCH_EFFICIENTNET_B3 ? build_graph_efficientnet(*n) : arch == HP_ARCH_RESNET50_FPN ? build_graph_r50fpn(*n)
                                                                                                    : build_graph(*n)) != HP_OK) {
    delete n;
    return nullptr;
  }
  return n;
}

// ---- HP_ARCH_CUSTOM: a feed-forward graph of convolutions described by the caller (the detector's RoI heads) ----
extern "C" int hp_net_add_conv(hp_net* net, const char* weight_name, const char* bias_name, int cin, int cout, int k, int stride,
                               int pad, int act, int H, int W, int in_slot, int out_slot, int res_slot) {
  HP_REQUIRE(net && net->arch == HP_ARCH_CUSTOM && !net->finalized, "hp_net_add_conv: needs an unfinalized HP_ARCH_CUSTOM network");
  HP_REQUIRE(weight_name && cin >= 1 && cout >= 1 && k >= 1 && (stride == 1 || stride == 2) && pad >= 0 && H >= 1 && W >= 1,
             "hp_net_add_conv: bad layer geometry");
  const bool gated = (act & HP_CONV_GATED) != 0;  // the input is multiplied by the gate of the squeeze-excitation op before it
  act &= ~HP_CONV_GATED;
  HP_REQUIRE(act >= HP_ACT_NONE && act <= HP_ACT_SWISH, "hp_net_add_conv: activation must be none, ReLU or swish");
  HP_REQUIRE(!gated || (k == 1 && cin % 4 == 0 && in_slot >= 0 && !net->ses.empty() && net->ses.back()->C == cin &&
                        net->ses.back()->in_buf == in_slot),
             "hp_net_add_conv: a gated layer is a 1x1 convolution on the slot the last hp_net_add_se pooled (cin % 4 == 0)");
  HP_REQUIRE(in_slot >= -1 && in_slot < 32 && out_slot >= 0 && out_slot < 32 && res_slot >= -1 && res_slot < 32 && out_slot != in_slot &&
                 out_slot != res_slot, "hp_net_add_conv: bad arena slots");
  HP_REQUIRE(in_slot >= 0 || (cin == net->n_inputs && H == net->h && W == net->w), "hp_net_add_conv: the first layer must match the network input");
  HP_REQUIRE((H + 2 * pad - k) / stride + 1 >= 1 && (W + 2 * pad - k) / stride + 1 >= 1, "hp_net_add_conv: empty output");
  const int cout4 = (cout + 3) / 4 * 4;  // rows rounded up to 4 (zero rows): outputs are read as [.., cout4]
  const int c = add_conv(*net, weight_name, "", "", cin, cout4, k, stride, pad, act, H, W, in_slot, out_slot, res_slot);
  ConvLayer& L = *net->convs[c];
  if (cout4 != cout) L.cout_real = cout;
  if (bias_name && bias_name[0]) L.bias_name = bias_name;
  if (gated) L.se = 1;
  want(*net, out_slot, (size_t)L.Ho * L.Wo * cout4);
  return HP_OK;
}

// The MBConv ops of build_graph_efficientnet for a caller-described graph: forward_chunk picks their launches (fused front,
// strip pooling, se_pool_kernel) as it does for the EfficientNet plan.
extern "C" int hp_net_add_dwconv(hp_net* net, const char* weight_name, const char* bn_prefix, int C, int k, int stride, int pad,
                                 int H, int W, int Ho, int Wo, int in_slot, int out_slot) {
  HP_REQUIRE(net && net->arch == HP_ARCH_CUSTOM && !net->finalized, "hp_net_add_dwconv: needs an unfinalized HP_ARCH_CUSTOM network");
  HP_REQUIRE(weight_name && bn_prefix && C >= 4 && C % 4 == 0 && (k == 3 || k == 5) && (stride == 1 || stride == 2) && pad >= 0 &&
                 pad < k && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "hp_net_add_dwconv: bad layer geometry");
  // the bottom / right padding the explicit output size implies: 0 .. k - 1 rows, like the top / left one
  const int hi_h = (Ho - 1) * stride + k - pad - H, hi_w = (Wo - 1) * stride + k - pad - W;
  HP_REQUIRE(hi_h >= 0 && hi_h < k && hi_w >= 0 && hi_w < k, "hp_net_add_dwconv: output size does not fit the input and the padding");
  HP_REQUIRE((int64_t)H * W * C * 4 < (int64_t)1 << 31 && (int64_t)Ho * Wo * C * 4 < (int64_t)1 << 31,
             "hp_net_add_dwconv: a map of one image exceeds the kernels' 32-bit offsets");
  HP_REQUIRE(in_slot >= -1 && in_slot < 32 && out_slot >= 0 && out_slot < 32 && out_slot != in_slot, "hp_net_add_dwconv: bad arena slots");
  if (in_slot < 0)
    HP_REQUIRE(C == net->c_pad && C == net->n_inputs && H == net->h && W == net->w, "hp_net_add_dwconv: the first layer must match the network input");
  else
    HP_REQUIRE(in_slot < (int)net->buf_floats_per_sample.size() && (size_t)H * W * C <= net->buf_floats_per_sample[in_slot],
               "hp_net_add_dwconv: the input slot is unwritten or smaller than the input map");
  net->bn_eps = 1e-3f;  // the BatchNorm of an MBConv block is EfficientNet's (hp_net_add_conv layers take no BatchNorm)
  add_dw(*net, weight_name, bn_prefix, C, k, stride, pad, H, W, Ho, Wo, in_slot, out_slot);
  want(*net, out_slot, (size_t)Ho * Wo * C);
  return HP_OK;
}

extern "C" int hp_net_add_se(hp_net* net, const char* prefix, int C, int Cse, int H, int W, int in_slot) {
  HP_REQUIRE(net && net->arch == HP_ARCH_CUSTOM && !net->finalized, "hp_net_add_se: needs an unfinalized HP_ARCH_CUSTOM network");
  HP_REQUIRE(prefix && C >= 4 && C % 4 == 0 && Cse >= 1 && Cse <= 128 && H >= 1 && W >= 1, "hp_net_add_se: bad layer geometry");
  HP_REQUIRE(in_slot >= 0 && in_slot < (int)net->buf_floats_per_sample.size() && (size_t)H * W * C <= net->buf_floats_per_sample[in_slot],
             "hp_net_add_se: the input slot is unwritten or smaller than the input map");
  add_se(*net, prefix, C, Cse, H * W, in_slot);
  return HP_OK;
}

extern "C" int hp_net_add_output(hp_net* net, int slot, int H, int W, int C) {
  HP_REQUIRE(net && net->arch == HP_ARCH_CUSTOM && !net->finalized, "hp_net_add_output: needs an unfinalized HP_ARCH_CUSTOM network");
  HP_REQUIRE(slot >= 0 && slot < (int)net->buf_floats_per_sample.size() && (size_t)H * W * C <= net->buf_floats_per_sample[slot],
             "hp_net_add_output: no such slot / shape larger than the slot");
  net->feature_maps.push_back({slot, H, W, C});
  return HP_OK;
}

extern "C" void hp_net_destroy(hp_net* net) {
  if (!net) return;
  for (auto& p : net->ev_pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
  for (auto& p : net->ev_pool) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
  delete net;
}

extern "C" int hp_net_input_channels_padded(const hp_net* net) { return net ? net->c_pad : HP_ERR_ARG; }

extern "C" int hp_net_set_param(hp_net* net, const char* name, const float* h_data, int64_t numel) {
  HP_REQUIRE(net && name && (h_data || numel == 0) && numel >= 0, "hp_net_set_param: bad argument");
  HP_REQUIRE(!net->finalized, "hp_net_set_param: network already finalized");
  net->params[name].assign(h_data, h_data + numel);
  return HP_OK;
}

// The tensors csrc/pool_head.hip reads as plain fp32 are stored as they were handed over: a copy on `stream` replaces one in a
// finalised network (no re-planning: the launch plan holds the buffers' addresses, which do not change).  Everything else was
// folded (BN into conv weights) or packed (tile order, fp16 splits, Winograd transforms) at finalise and is refused.
static int head_param(hp_net* net, const char* name, int64_t numel, const char* what, DevBuf** buf) {
  HP_REQUIRE(net && name, std::string(what) + ": bad argument");
  HP_REQUIRE(net->finalized, std::string(what) + ": network not finalized (hp_net_set_param takes host data before that)");
  const std::string k(name);
  const int64_t C = net->n_features;
  DevBuf* dst = nullptr;
  int64_t want = 0;
  if (k == "pose_fc.weight") { dst = &net->pose_w; want = net->pose_dim * C; }
  else if (k == "pose_fc.bias") { dst = &net->pose_b; want = net->pose_dim; }
  else if (k == "views_logits_head.weight") { dst = &net->logit_w; want = net->n_logits * C; }
  else if (k == "views_logits_head.bias") { dst = &net->logit_b; want = net->n_logits; }
  else if (k == "backbone.fc.weight") { dst = &net->fc_w; want = 512 * 512; }
  else if (k == "backbone.fc.bias") { dst = &net->fc_b; want = 512; }
  else
    return fail(HP_ERR_ARG, std::string(what) + ": '" + k + "' is folded or packed at finalise; only the head tensors (pose_fc, "
                            "views_logits_head, backbone.fc) are kept as plain fp32 in a finalised network");
  HP_REQUIRE(dst->p && want > 0, std::string(what) + ": the network has no '" + k + "'");
  HP_REQUIRE(numel == want, std::string(what) + ": '" + k + "' has " + std::to_string(want) + " elements, got " + std::to_string(numel));
  *buf = dst;
  return HP_OK;
}

extern "C" int hp_net_set_param_device(hp_net* net, const char* name, const float* d_data, int64_t numel, void* stream) {
  HP_REQUIRE(d_data, "hp_net_set_param_device: null data");
  DevBuf* buf = nullptr;
  int rc = head_param(net, name, numel, "hp_net_set_param_device", &buf);
  if (rc) return rc;
  HP_CHECK_HIP(hipMemcpyAsync(buf->p, d_data, (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return HP_OK;
}

extern "C" int hp_net_get_param_device(hp_net* net, const char* name, float* d_data, int64_t numel, void* stream) {
  HP_REQUIRE(d_data, "hp_net_get_param_device: null data");
  DevBuf* buf = nullptr;
  int rc = head_param(net, name, numel, "hp_net_get_param_device", &buf);
  if (rc) return rc;
  HP_CHECK_HIP(hipMemcpyAsync(d_data, buf->p, (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return HP_OK;
}

extern "C" int hp_net_set_pooled_out(hp_net* net, float* d_pooled) {
  HP_REQUIRE(net && net->finalized, "hp_net_set_pooled_out: network not finalized");
  HP_REQUIRE(!d_pooled || net->fc_w.p, "hp_net_set_pooled_out: the network has no fc in front of its heads");
  net->pooled_out = d_pooled;
  return HP_OK;
}

extern "C" int hp_net_set_precision(hp_net* net, int precision) {
  HP_REQUIRE(net, "hp_net_set_precision: null net");
  HP_REQUIRE(!net->finalized, "hp_net_set_precision: network already finalized");
  HP_REQUIRE(precision == HP_PRECISION_F32 || precision == HP_PRECISION_F16, "hp_net_set_precision: unknown precision");
  net->precision = precision;
  return HP_OK;
}

extern "C" int hp_net_precision(const hp_net* net) { return net ? net->precision : HP_ERR_ARG; }

extern "C" int hp_net_output_dims(const hp_net* net, int* pose_dim, int* n_logits, int* n_features) {
  HP_REQUIRE(net && net->finalized, "hp_net_output_dims: network not finalized");
  if (pose_dim) *pose_dim = net->pose_dim;
  if (n_logits) *n_logits = net->n_logits;
  if (n_features) *n_features = net->n_features;
  return HP_OK;
}

extern "C" int hp_net_input_dims(const hp_net* net, int* h, int* w, int* c_pad, int* device) {
  HP_REQUIRE(net, "hp_net_input_dims: null network");
  if (h) *h = net->h;
  if (w) *w = net->w;
  if (c_pad) *c_pad = net->c_pad;
  if (device) *device = net->device;
  return HP_OK;
}

extern "C" int hp_net_finalize(hp_net* net, int max_batch) {
  HP_REQUIRE(net && max_batch >= 1, "hp_net_finalize: bad argument");
  int rc = conv_setup_once();
  if (rc) return rc;
  const bool f16 = net->precision == HP_PRECISION_F16;
  HP_REQUIRE(!(f16 && (net->arch == HP_ARCH_EFFICIENTNET_B3 || net->arch == HP_ARCH_RESNET50_FPN)),
             "hp_net_finalize: no fp16 plan for EfficientNet / the detector backbone");
  for (auto& D : net->dws)
    if ((rc = pack_dw(*net, *D))) return rc;
  for (auto& S : net->ses)
    if ((rc = pack_se(*net, *S))) return rc;
  if (net->se_max_c > 0) {
    if ((rc = net->se_pooled.alloc((size_t)max_batch * net->se_max_c * 4))) return rc;
    if ((rc = net->se_gate.alloc((size_t)max_batch * net->se_max_c * 4))) return rc;
    if ((rc = net->se_sq.alloc((size_t)max_batch * 128 * 4))) return rc;
    size_t part = (size_t)se_partial_floats(max_batch, net->se_max_c);
    for (auto& D : net->dws)  // the fused front launch leaves one partial per tile of its output
      part = std::max(part, (size_t)max_batch * mbconv_front_tiles(D->Ho, D->Wo, D->stride) * D->C);
    if ((rc = net->se_partial.alloc(part * 4))) return rc;
  }
  for (auto& L : net->convs)
    if ((rc = f16 ? pack_conv_f16(*net, *L) : pack_conv(*net, *L))) return rc;
  const std::vector<float>* v;
  if (net->arch == HP_ARCH_VANILLA_RESNET34) {
    if ((rc = need(*net, "backbone.fc.weight", 512 * 512, &v))) return rc;
    if ((rc = net->fc_w.upload(v->data(), v->size() * 4))) return rc;
    if ((rc = need(*net, "backbone.fc.bias", 512, &v))) return rc;
    if ((rc = net->fc_b.upload(v->data(), v->size() * 4))) return rc;
    if ((rc = net->head_ws.alloc((size_t)2 * max_batch * 512 * 4))) return rc;
  }
  net->pose_dim = net->n_logits = 0;
  if ((v = find(*net, "pose_fc.weight"))) {
    HP_REQUIRE(v->size() % net->n_features == 0 && !v->empty(), "pose_fc.weight must be [pose_dim, n_features]");
    net->pose_dim = (int)(v->size() / net->n_features);
    if ((rc = net->pose_w.upload(v->data(), v->size() * 4))) return rc;
    if ((rc = need(*net, "pose_fc.bias", net->pose_dim, &v))) return rc;
    if ((rc = net->pose_b.upload(v->data(), v->size() * 4))) return rc;
  }
  if ((v = find(*net, "views_logits_head.weight"))) {
    HP_REQUIRE(v->size() % net->n_features == 0 && !v->empty(), "views_logits_head.weight must be [n_views, n_features]");
    net->n_logits = (int)(v->size() / net->n_features);
    if ((rc = net->logit_w.upload(v->data(), v->size() * 4))) return rc;
    if ((rc = need(*net, "views_logits_head.bias", net->n_logits, &v))) return rc;
    if ((rc = net->logit_b.upload(v->data(), v->size() * 4))) return rc;
  }
  net->bufs.clear();
  net->bufs.resize(net->buf_floats_per_sample.size());
  for (size_t s = 0; s < net->bufs.size(); ++s)
    if ((rc = net->bufs[s].alloc(net->buf_floats_per_sample[s] * (size_t)max_batch * (f16 ? 2 : 4)))) return rc;
  if (f16 && (rc = net->x16.alloc((size_t)max_batch * net->h * net->w * net->convs[0]->cin16 * 2))) return rc;
  if (!net->h_status) {
    HP_CHECK_HIP(hipHostMalloc((void**)&net->h_status, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *net->h_status = 0u;
    HP_CHECK_HIP(hipHostGetDevicePointer((void**)&net->d_status, net->h_status, 0));
  }
  { int rc_a = net->amax.alloc((net->ops.size() + 1) * (size_t)kAmaxSlots * kAmaxStride * sizeof(unsigned)); if (rc_a) return rc_a; }
  net->max_batch = max_batch;
  net->taps.clear();
  net->op_path.assign(net->ops.size(), HP_PATH_NONE);
  net->op_mat.assign(net->ops.size(), 0);
  net->params.clear();  // host copies are no longer needed
  net->finalized = true;
  return HP_OK;
}

// Builds the Winograd weight sets a forward under `algo` can reach and that do not exist yet (see pack_conv): allocation
// plus a transform launch on `stream`, i.e. ordered before the forward's own launches.  Not possible while the stream
// captures (hipMalloc): the Python layer runs the first call after an algorithm switch eagerly (ops.bump_graph_epoch).
static int ensure_wino_weights(hp_net* net, int algo, hipStream_t stream) {
  const bool exact = algo == HP_CONV_ALGO_WINOGRAD_1WAVE || algo == HP_CONV_ALGO_WINOGRAD;
  int rc;
  bool capturing_checked = false;
  auto can_build = [&]() -> int {
    if (capturing_checked) return HP_OK;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HP_CHECK_HIP(hipStreamIsCapturing(stream, &st));
    if (st != hipStreamCaptureStatusNone)
      return fail(HP_ERR_ARG, "hp_net_forward: Winograd weights of this algorithm are not built yet; run one eager forward before capturing");
    capturing_checked = true;
    return HP_OK;
  };
  for (auto& Lp : net->convs) {
    ConvLayer& L = *Lp;
    // exact-fp32 set: the Winograd algorithms, and under AUTO the layers without split-fp16 weights
    if (L.sets.wino && !L.w_wino.p && (exact || (algo == HP_CONV_ALGO_AUTO && !L.sets.split))) {
      if ((rc = can_build())) return rc;
      if ((rc = L.w_wino.alloc(conv_wino_weight_floats(L.cout, L.cin) * 4))) return rc;
      if ((rc = conv_wino_transform_weights((const float*)L.w.p, (float*)L.w_wino.p, L.cout, L.cin, L.Kpad, stream))) return rc;
    }
  }
  return HP_OK;
}

namespace hp {
namespace {

// One chunk of a forward: what the op bodies below share, and the state carried from op to op.
struct Chunk {
  Net& net;
  const float* d_x;    // fp32 input [batch][h][w][c_pad]; or (fp16 plan only)
  const void* d_x16;   // fp16 input [batch][h][w][cin16 of the stem]
  int b0, batch;       // b0 = index of the chunk's first sample in the caller's batch (tap offsets; b0 == 0 starts the launch-path record)
  float *d_pose, *d_logits, *d_features;
  hipStream_t stream;
  bool f16, sync_ops /* diagnostics: fault isolation */, per_launch, no_sc_fusion /* HP_NET_NO_SHORTCUT_FUSION=1: separate launches */;
  int algo;
  unsigned* amax_words;
  bool pool_fused = false;   // the stem wrote the pooled map itself: skip the max-pool op that follows it
  bool front_fused = false;  // the expansion conv ran the depthwise conv after it too (mbconv_front.hip): skip that op
  int dw_partials = 0;       // > 0: the depthwise launch left this many pooling partials per image for the SE op after it
  int sc_done = -1;          // op index of a shortcut the 3x3 op before it has already run
  std::vector<int> buf_amax; // arena slot -> op whose launch tracked max|y| of what it holds (-1: unknown)
  // profiling: events are recorded on the launch stream and only READ in hp_net_profile_collect
  EventPair run{};
  bool run_open = false;

  int prof_begin(int conv) {
    if (!net.profiling || run_open) return HP_OK;
    if (!net.ev_pool.empty()) { run = net.ev_pool.back(); net.ev_pool.pop_back(); }
    else { run = EventPair{}; HP_CHECK_HIP(hipEventCreate(&run.e0)); HP_CHECK_HIP(hipEventCreate(&run.e1)); }
    run.flops = run.mfma_flops = 0.0; run.n = 0; run.conv = per_launch ? conv : -1;
    HP_CHECK_HIP(hipEventRecord(run.e0, stream));
    run_open = true;
    return HP_OK;
  }
  void prof_add(double flops, double mfma_flops) { if (run_open) { run.flops += flops; run.mfma_flops += mfma_flops; ++run.n; } }
  int prof_end(bool force) {
    if (!run_open || !(force || per_launch)) return HP_OK;
    HP_CHECK_HIP(hipEventRecord(run.e1, stream));
    net.ev_pending.push_back(run);
    run_open = false;
    return HP_OK;
  }
  // host-side record of what this forward launched for op i (hp_net_op_info); a later chunk that differs marks it MIXED
  void note(size_t i, int path, bool materialised = true) {
    if (b0 == 0) { net.op_path[i] = path; net.op_mat[i] = materialised; return; }
    if (net.op_path[i] != path) net.op_path[i] = HP_PATH_MIXED;
    net.op_mat[i] = net.op_mat[i] && materialised;
  }
  int tap(size_t i, bool materialised) {  // copy op i's output map of this chunk to its tap
    void* dst = net.taps[i];
    if (!dst || !materialised) return HP_OK;
    const Op& o = net.ops[i];
    const size_t elem = f16 ? 2 : 4;
    int slot = o.out_buf;
    size_t per_sample = (size_t)o.Ho * o.Wo * o.C;
    if (o.kind == OP_CONV) { const ConvLayer& L = *net.convs[o.conv]; slot = L.out_buf; per_sample = (size_t)L.Ho * L.Wo * L.cout; }
    else if (o.kind == OP_DW) { const DwLayer& D = *net.dws[o.conv]; slot = D.out_buf; per_sample = (size_t)D.Ho * D.Wo * D.C; }
    HP_CHECK_HIP(hipMemcpyAsync((char*)dst + (size_t)b0 * per_sample * elem, net.bufs[slot].p, (size_t)batch * per_sample * elem,
                                hipMemcpyDeviceToDevice, stream));
    return HP_OK;
  }
  unsigned* amax_of(size_t op) const { return amax_words + op * (size_t)kAmaxSlots * kAmaxStride; }
  const Op* next_op(size_t oi) const { return oi + 1 < net.ops.size() ? &net.ops[oi + 1] : nullptr; }
};

// Every body: the launches of op oi of this chunk; `written` = the op's output map exists after its turn.

int op_conv_f16(Chunk& c, size_t oi, bool& written) {
  Net& net = c.net; const Op& op = net.ops[oi]; ConvLayer& L = *net.convs[op.conv]; int rc;
  ConvArgsH a{};
  a.x = (const _Float16*)(L.in_buf < 0 ? c.d_x16 : net.bufs[L.in_buf].p);
  a.w = (const _Float16*)L.w16.p;
  a.bias = (const float*)L.bias.p;
  a.residual = L.res_buf < 0 ? nullptr : (const _Float16*)net.bufs[L.res_buf].p;
  a.pre_scale = (const _Float16*)L.pre_scale16.p;
  a.pre_shift = (const _Float16*)L.pre_shift16.p;
  a.lut = (const int4*)L.lut16.p;
  a.y = (_Float16*)net.bufs[L.out_buf].p;
  a.M = (int64_t)c.batch * L.Ho * L.Wo;
  a.H = L.H; a.W = L.W; a.Cin = L.cin16; a.Ho = L.Ho; a.Wo = L.Wo; a.Cout = L.cout;
  a.stride = L.stride; a.pad = L.pad; a.Kpad = L.Kpad16; a.ktiles = L.Kpad16 / 64; a.relu = L.relu;
  a.kh = L.kh; a.kw = L.kw;
  a.no_tail_split = net.tail_split ? 0 : 1;
  a.status = net.d_status;  // every fp16 launch that writes activations reports into the network's guard word
  a.x_bytes = (int64_t)c.batch * L.H * L.W * L.cin16 * 2;
  a.w_bytes = (int64_t)L.cout * L.Kpad16 * 2;
  if ((rc = c.prof_begin(op.conv))) return rc;
  const Op* next = c.next_op(oi);
  if (L.w_stem7.p && next && next->kind == OP_MAXPOOL && next->in_buf == L.out_buf && next->H == L.Ho && next->W == L.Wo) {
    // stem + ReLU + max-pool in one launch (conv_stem7.hip): the conv map is never written
    ConvArgs s7{};
    s7.x = (const float*)a.x; s7.w = (const float*)L.w_stem7.p; s7.bias = a.bias; s7.y = (float*)net.bufs[next->out_buf].p;
    s7.M = a.M; s7.H = L.H; s7.W = L.W; s7.Cin = L.cin16; s7.Ho = L.Ho; s7.Wo = L.Wo; s7.Cout = L.cout; s7.relu = L.relu;
    s7.Kpad = L.cin_real;  // selects the kernel the weights were packed for
    s7.status = a.status;
    if ((rc = launch_conv_stem7_pool(s7, 1, c.stream))) return rc;
    c.pool_fused = true; written = false;
    c.note(oi, HP_PATH_STEM7_POOL_F16, false);
    c.prof_add(2.0 * (double)a.M * L.cout * L.kh * L.kw * L.cin_real, 2.0 * (double)a.M * (256.0 / 192.0) * L.cout * 7 * conv_stem7_f16_krow(L.cin_real));
  } else {
    if ((rc = launch_conv_f16(a, c.stream))) return rc;
    c.note(oi, HP_PATH_CONV_F16);
    c.prof_add(2.0 * (double)a.M * L.cout * L.kh * L.kw * L.cin_real, 2.0 * (double)((a.M + 127) / 128 * 128) * L.cout * L.Kpad16);
  }
  return c.prof_end(false);
}

// May op oi + 1 ride in the launch of op oi, as the 1x1 / stride-2 shortcut of the block whose 3x3 / stride-2 conv op oi is?
// The structure only (the plans put the shortcut right behind the 3x3 op); the diagnostics and the launch limits are
// choose_conv's.  B.w_short exists only where the persistent stride-2 kernel takes this geometry (conv_weight_sets).
bool shortcut_may_ride(const Net& net, size_t oi) {
  if (oi + 1 >= net.ops.size() || net.ops[oi + 1].kind != OP_CONV) return false;
  const ConvLayer& A = *net.convs[net.ops[oi].conv];
  const ConvLayer& B = *net.convs[net.ops[oi + 1].conv];
  if (!B.w_short.p || !A.w_split.p || A.kh != 3 || A.kw != 3 || A.stride != 2 || A.pad != 1 || A.res_buf >= 0 || A.se) return false;
  if (A.in_buf != B.in_buf || A.cin != B.cin || A.cout != B.cout || A.H != B.H || A.W != B.W || A.Ho != B.Ho || A.Wo != B.Wo) return false;
  return A.bn_before == B.bn_before && A.out_buf != B.out_buf;  // one staging prologue serves both
}

int op_conv(Chunk& c, size_t oi, bool& written) {
  Net& net = c.net;
  const Op& op = net.ops[oi];
  if ((int)oi == c.sc_done) {
    c.sc_done = -1;  // this shortcut rode in the previous op's launch
    c.note(oi, HP_PATH_RODE);
    return HP_OK;
  }
  ConvLayer& L = *net.convs[op.conv];
  int rc;
  ConvArgs a{};
  a.x = L.in_buf < 0 ? c.d_x : (const float*)net.bufs[L.in_buf].p;
  a.bias = (const float*)L.bias.p;
  a.residual = L.res_buf < 0 ? nullptr : (const float*)net.bufs[L.res_buf].p;
  a.pre_scale = (const float*)L.pre_scale.p;
  a.pre_shift = (const float*)L.pre_shift.p;
  a.lut = (const int4*)L.lut.p;
  a.y = (float*)net.bufs[L.out_buf].p;
  a.M = (int64_t)c.batch * L.Ho * L.Wo;
  a.H = L.H; a.W = L.W; a.Cin = L.cin; a.Ho = L.Ho; a.Wo = L.Wo; a.Cout = L.cout;
  a.stride = L.stride; a.pad = L.pad; a.Kpad = L.Kpad; a.ktiles = L.Kpad / 32; a.relu = L.relu;
  a.algo = c.algo; a.no_tail_split = net.tail_split ? 0 : 1;
  if (c.amax_words) {
    if (L.in_buf >= 0 && c.buf_amax[L.in_buf] >= 0 && !L.se) {
      a.amax_in = c.amax_of(c.buf_amax[L.in_buf]);
      a.amax_a = L.pre_scale.p ? L.pre_smax : 1.f; a.amax_b = L.pre_scale.p ? L.pre_bmax : 0.f;
    }
    a.amax_out = c.amax_of(oi);
  }
  if (L.se) { a.pre_scale = (const float*)net.se_gate.p; a.pre_shift = nullptr; }  // gate [batch][Cin]
  if (c.sync_ops)
    std::fprintf(stderr, "[hp net]   conv %s M=%lld H=%d W=%d Cin=%d Ho=%d Wo=%d Cout=%d pad=%d Kpad=%d act=%d se=%d in=%d out=%d res=%d x=%p y=%p r=%p\n",
                 L.wname.c_str(), (long long)a.M, a.H, a.W, a.Cin, a.Ho, a.Wo, a.Cout, a.pad, a.Kpad, a.relu, L.se, L.in_buf,
                 L.out_buf, L.res_buf, (const void*)a.x, (void*)a.y, (const void*)a.residual);
  if ((rc = c.prof_begin(op.conv))) return rc;
  // the site: the layer, the sets it has by now, and what its neighbours allow
  ConvSite s = layer_site(L);
  s.bias = a.bias != nullptr;
  s.has_split = L.w_split.p != nullptr; s.has_isplit = L.w_isplit.p != nullptr; s.has_wino = L.w_wino.p != nullptr; s.has_stem7 = L.w_stem7.p != nullptr;
  s.algo = c.algo; s.batch = c.batch;
  const Op* next = c.next_op(oi);
  s.pool_follows = next && next->kind == OP_MAXPOOL && next->in_buf == L.out_buf && next->H == L.Ho && next->W == L.Wo;
  const DwLayer* dw = nullptr;
  if (oi + 2 < net.ops.size() && next->kind == OP_DW && net.ops[oi + 2].kind == OP_SE) {
    const DwLayer& D = *net.dws[next->conv];
    if (D.in_buf == L.out_buf && D.C == L.cout && D.H == L.Ho && D.W == L.Wo && net.ses[net.ops[oi + 2].conv]->in_buf == D.out_buf) {
      dw = &D;
      s.dw_se_follow = true; s.dw_k = D.k; s.dw_stride = D.stride; s.dw_Ho = D.Ho; s.dw_Wo = D.Wo;
    }
  }
  s.shortcut_follows = shortcut_may_ride(net, oi);
  s.per_launch = c.per_launch; s.sync_ops = c.sync_ops; s.no_sc_fusion = c.no_sc_fusion;
  const ConvChoice ch = choose_conv(s);

  const void* const sets[] = {L.w.p, L.w_split.p, L.w_isplit.p, L.w_wino.p, L.w_stem7.p};  // by WeightSet
  a.w = (const float*)sets[ch.w];
  if (ch.status) a.status = net.d_status;
  if (ch.pool_fused) a.y = (float*)net.bufs[next->out_buf].p;  // the pooled map: the conv map is never written
  switch (ch.path) {
    case HP_PATH_MBCONV_FRONT: {
      FrontArgs f{};
      f.x = a.x; f.w_split = a.w; f.bias_e = a.bias; f.w_dw = (const float*)dw->w.p; f.bias_d = (const float*)dw->bias.p;
      f.y = (float*)net.bufs[dw->out_buf].p; f.pool_partial = (float*)net.se_partial.p; f.status = net.d_status;
      f.n = c.batch; f.H = L.H; f.W = L.W; f.Cin = L.cin; f.Cexp = L.cout; f.Ho = dw->Ho; f.Wo = dw->Wo; f.k = dw->k;
      f.stride = dw->stride; f.pad_t = f.pad_l = dw->pad; f.Kpad = L.Kpad; f.rows_pad = L.cout_pad;
      rc = launch_mbconv_front(f, c.stream);
      c.buf_amax[dw->out_buf] = -1;
      c.dw_partials = mbconv_front_tiles(dw->Ho, dw->Wo, dw->stride);
      break;
    }
    case HP_PATH_STEM7_POOL: rc = launch_conv_stem7_pool(a, 0, c.stream); break;
    case HP_PATH_SPLIT3X3_SHORTCUT: {  // the block's shortcut as extra work items of this launch
      const int sc_op = (int)oi + 1;
      const ConvLayer& S = *net.convs[net.ops[sc_op].conv];
      c.sc_done = sc_op;
      a.sc_w = (const float*)S.w_short.p; a.sc_bias = (const float*)S.bias.p; a.sc_y = (float*)net.bufs[S.out_buf].p;
      a.sc_relu = S.relu;
      a.sc_amax_out = c.amax_words ? c.amax_of(sc_op) : nullptr;
      if (S.out_buf >= 0) c.buf_amax[S.out_buf] = c.amax_words ? sc_op : -1;
      c.prof_add(2.0 * (double)a.M * S.cout * S.cin_real, ch.sc_mfma_flops);
    }
      [[fallthrough]];
    case HP_PATH_SPLIT3X3: rc = launch_conv_split(a, c.stream); break;
    case HP_PATH_WINOGRAD: rc = launch_conv_wino(a, c.stream); break;
    case HP_PATH_STEM_SPLIT_POOL: rc = launch_conv_stem_split_pool(a, c.stream); break;
    case HP_PATH_IGEMM_SPLIT_POOL: rc = launch_conv_igemm_split_pool(a, c.stream); break;
    case HP_PATH_IGEMM_SPLIT: rc = launch_conv_igemm_split(a, ch.variant, c.stream); break;
    case HP_PATH_PATCH: rc = launch_conv_patch(a, ch.variant, c.stream); break;
    default: rc = launch_conv(a, ch.variant, c.stream); break;
  }
  c.pool_fused = ch.pool_fused; c.front_fused = ch.front_fused; written = ch.materialised;
  c.note(oi, ch.path, ch.materialised);
  if (rc) return rc;
  if (L.out_buf >= 0) c.buf_amax[L.out_buf] = c.amax_words && ch.tracks_amax ? (int)oi : -1;
  if (ch.pool_fused && next->out_buf >= 0) c.buf_amax[next->out_buf] = -1;  // the fused stems write the pooled map untracked
  c.prof_add(2.0 * (double)a.M * L.cout * L.kh * L.kw * L.cin_real, ch.mfma_flops);
  return c.prof_end(false);
}

int op_dw(Chunk& c, size_t oi, bool&) {
  Net& net = c.net; int rc;
  if (c.front_fused) {
    c.front_fused = false;  // the expansion's launch wrote this depthwise output (and the pooling partials) already
    c.note(oi, HP_PATH_FUSED_AWAY);
    return c.prof_end(true);
  }
  if ((rc = c.prof_end(true))) return rc;
  const DwLayer& D = *net.dws[net.ops[oi].conv];
  c.buf_amax[D.out_buf] = -1;  // the depthwise kernels do not track their range
  DwArgs d{};
  d.x = D.in_buf < 0 ? c.d_x : (const float*)net.bufs[D.in_buf].p; d.w = (const float*)D.w.p; d.bias = (const float*)D.bias.p;
  d.y = (float*)net.bufs[D.out_buf].p;
  d.n = c.batch; d.H = D.H; d.W = D.W; d.C = D.C; d.Ho = D.Ho; d.Wo = D.Wo; d.k = D.k; d.stride = D.stride;
  d.pad_t = d.pad_l = D.pad;
  // the squeeze-excitation that follows pools this output: let the depthwise launch sum what it stores
  c.dw_partials = 0;
  const Op* next = c.next_op(oi);
  if (next && next->kind == OP_SE && net.ses[next->conv]->in_buf == D.out_buf && dwconv_pools(d) &&
      dwconv_pool_strips(D.Ho, D.k, D.stride) <= 32) {
    d.pool_partial = (float*)net.se_partial.p;
    c.dw_partials = dwconv_pool_strips(D.Ho, D.k, D.stride);
  }
  if ((rc = launch_dwconv(d, c.stream))) return rc;
  c.note(oi, HP_PATH_DWCONV);
  return HP_OK;
}

int op_se(Chunk& c, size_t oi, bool& written) {
  Net& net = c.net; int rc;
  if ((rc = c.prof_end(true))) return rc;
  const SeLayer& S = *net.ses[net.ops[oi].conv];
  if ((rc = launch_se((const float*)net.bufs[S.in_buf].p, (float*)net.se_partial.p, (float*)net.se_pooled.p, (float*)net.se_sq.p,
                      (float*)net.se_gate.p, (const float*)S.w1.p, (const float*)S.b1.p, (const float*)S.w2.p, (const float*)S.b2.p,
                      c.batch, S.HW, S.C, S.Cse, c.dw_partials, c.stream)))
    return rc;
  c.dw_partials = 0; written = false;
  c.note(oi, HP_PATH_SE, false);
  return HP_OK;
}

int op_resize(Chunk& c, size_t oi, bool&) {
  Net& net = c.net; const Op& op = net.ops[oi]; int rc;
  c.buf_amax[op.out_buf] = -1;
  if ((rc = c.prof_end(true))) return rc;
  if ((rc = launch_resize_nearest((const float*)net.bufs[op.in_buf].p, (float*)net.bufs[op.out_buf].p, c.batch, op.H, op.W,
                                  op.C, op.Ho, op.Wo, op.conv, c.stream)))
    return rc;
  c.note(oi, HP_PATH_RESIZE);
  return HP_OK;
}

int op_maxpool(Chunk& c, size_t oi, bool&) {
  Net& net = c.net; const Op& op = net.ops[oi]; int rc;
  if (c.pool_fused) {
    c.pool_fused = false;
    c.note(oi, HP_PATH_FUSED_AWAY);
    return c.prof_end(true);
  }
  if ((rc = c.prof_end(true))) return rc;
  if (c.f16) {
    if ((rc = launch_maxpool_f16(net.bufs[op.in_buf].p, net.bufs[op.out_buf].p, c.batch, op.H, op.W, op.C, op.Ho, op.Wo, c.stream)))
      return rc;
    c.note(oi, HP_PATH_MAXPOOL_F16);
    return HP_OK;
  }
  c.buf_amax[op.out_buf] = c.buf_amax[op.in_buf];  // a max over windows cannot exceed the input's largest magnitude
  if ((rc = launch_maxpool((const float*)net.bufs[op.in_buf].p, (float*)net.bufs[op.out_buf].p, c.batch, op.H, op.W, op.C, op.Ho,
                           op.Wo, c.stream)))
    return rc;
  c.note(oi, HP_PATH_MAXPOOL);
  return HP_OK;
}

int op_head(Chunk& c, size_t oi, bool& written) {
  Net& net = c.net; const Op& op = net.ops[oi]; int rc;
  if ((rc = c.prof_end(true))) return rc;
  // (fp16 plan: the head reads halves that the last conv stored and reported on, and accumulates in fp32: no guard of its own)
  HeadArgs h{};
  h.x = net.bufs[op.in_buf].p; h.x_is_half = c.f16 ? 1 : 0; h.HW = op.H * op.W; h.C = op.C;
  h.fc_w = (const float*)net.fc_w.p; h.fc_b = (const float*)net.fc_b.p;
  h.pose_w = (const float*)net.pose_w.p; h.pose_b = (const float*)net.pose_b.p;
  h.pose_dim = c.d_pose ? net.pose_dim : 0;
  h.logit_w = (const float*)net.logit_w.p; h.logit_b = (const float*)net.logit_b.p;
  h.n_logits = c.d_logits ? net.n_logits : 0;
  h.pose_out = c.d_pose; h.logit_out = c.d_logits; h.features = c.d_features;
  h.ws_pool = (float*)net.head_ws.p; h.ws_fc = h.ws_pool ? h.ws_pool + (size_t)net.max_batch * 512 : nullptr;
  if ((rc = launch_head(h, c.batch, c.stream))) return rc;
  if (net.pooled_out && h.ws_pool)
    HP_CHECK_HIP(hipMemcpyAsync(net.pooled_out + (size_t)c.b0 * 512, h.ws_pool, (size_t)c.batch * 512 * 4, hipMemcpyDeviceToDevice, c.stream));
  written = false;
  c.note(oi, HP_PATH_HEAD, false);
  return HP_OK;
}

}  // namespace
}  // namespace hp

static int forward_chunk(hp_net* net, const float* d_x, const void* d_x16, int b0, int batch, float* d_pose, float* d_logits,
                         float* d_features, hipStream_t stream) {
  int rc;
  const bool f16 = net->precision == HP_PRECISION_F16;
  if (f16 && !d_x16) {
    if ((rc = launch_cast_pad_f16(d_x, net->x16.p, (int64_t)batch * net->h * net->w, net->c_pad, net->convs[0]->cin16, stream)))
      return rc;
    d_x16 = net->x16.p;
  }
  // the guard of an EARLIER forward fired (read without synchronising): from now on exact-fp32 kernels only
  // (not while `stream` is capturing: the exact set may still have to be BUILT -- ensure_wino_weights allocates -- and a
  // capture must record the kernels of the signature it was started for; the flag is adopted by the next eager forward or
  // by hp_net_status, which the predictors call after every step and which drops the captured graphs)
  if (net->h_status && *(volatile unsigned*)net->h_status) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing((hipStream_t)stream, &cap);
    // (an fp16 network has no exact kernels of its own and never latches: its flag is the caller's to act on, hp_net_status)
    if (cap == hipStreamCaptureStatusNone && !f16) net->exact_only = true;
  }
  const int net_algo = net->exact_only ? HP_CONV_ALGO_WINOGRAD : (net->algo >= 0 ? net->algo : HP_CONV_ALGO_AUTO);
  if (!f16 && (rc = ensure_wino_weights(net, net_algo, stream))) return rc;
  unsigned* const amax_words = (f16 || !net->act_scale) ? nullptr : (unsigned*)net->amax.p;
  if (amax_words && (rc = launch_zero_words(amax_words, ((int)net->ops.size() + 1) * kAmaxSlots * kAmaxStride, stream))) return rc;
  Chunk c{*net, d_x, d_x16, b0, batch, d_pose, d_logits, d_features, stream, f16, dbg(DBG_NET_SYNC) != 0,
          dbg(DBG_PROFILE_LAYERS) != 0, dbg(DBG_NET_NO_SHORTCUT_FUSION) != 0, net_algo, amax_words};
  c.buf_amax.assign(net->bufs.size(), -1);
  for (size_t oi = 0; oi < net->ops.size(); ++oi) {
    const Op& op = net->ops[oi];
    bool written = true;
    if (c.sync_ops) {
      HP_CHECK_HIP(hipDeviceSynchronize());
      std::fprintf(stderr, "[hp net] op %d kind %d conv %d (everything before it has completed)\n", (int)oi, (int)op.kind, op.conv);
    }
    switch (op.kind) {
      case OP_CONV: rc = f16 ? op_conv_f16(c, oi, written) : op_conv(c, oi, written); break;
      case OP_DW: rc = op_dw(c, oi, written); break;
      case OP_SE: rc = op_se(c, oi, written); break;
      case OP_RESIZE: rc = op_resize(c, oi, written); break;
      case OP_MAXPOOL: rc = op_maxpool(c, oi, written); break;
      default: rc = op_head(c, oi, written); break;
    }
    if (rc) return rc;
    if (!net->taps.empty() && (rc = c.tap(oi, written))) return rc;
  }
  return c.prof_end(true);
}

// taps copy into caller-owned memory at addresses that belong to one forward: not while `stream` captures
static int taps_allowed(hp_net* net, hipStream_t stream) {
  if (net->taps.empty()) return HP_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  HP_CHECK_HIP(hipStreamIsCapturing(stream, &st));
  if (st != hipStreamCaptureStatusNone) return fail(HP_ERR_ARG, "hp_net_forward: taps are set (hp_net_set_taps) and the stream is capturing");
  return HP_OK;
}

extern "C" int hp_net_forward(hp_net* net, const float* d_x, int batch, float* d_pose, float* d_logits,
                              float* d_features, void* stream) {
  HP_REQUIRE(net && net->finalized, "hp_net_forward: network not finalized");
  HP_REQUIRE(batch >= 0, "hp_net_forward: negative batch");
  if (batch == 0) return HP_OK;
  HP_REQUIRE(d_x, "hp_net_forward: null input");
  HP_REQUIRE(!d_pose || net->pose_dim > 0, "hp_net_forward: network has no pose head");
  HP_REQUIRE(!d_logits || net->n_logits > 0, "hp_net_forward: network has no logits head");
  HP_REQUIRE(net->feature_maps.empty() || (batch <= net->max_batch && !d_pose && !d_logits && !d_features),
             "hp_net_forward: a feature-pyramid network takes at most max_batch images and has no heads (hp_net_feature_map)");
  hipStream_t st = (hipStream_t)stream;
  int rc_t = taps_allowed(net, st);
  if (rc_t) return rc_t;
  const size_t in_stride = (size_t)net->h * net->w * net->c_pad;
  for (int b0 = 0; b0 < batch; b0 += net->max_batch) {
    const int nb = batch - b0 < net->max_batch ? batch - b0 : net->max_batch;
    int rc = forward_chunk(net, d_x + (size_t)b0 * in_stride, nullptr, b0, nb,
                           d_pose ? d_pose + (size_t)b0 * net->pose_dim : nullptr,
                           d_logits ? d_logits + (size_t)b0 * net->n_logits : nullptr,
                           d_features ? d_features + (size_t)b0 * net->n_features : nullptr, st);
    if (rc) return rc;
  }
  return HP_OK;
}

extern "C" int hp_net_n_feature_maps(const hp_net* net) { return net ? (int)net->feature_maps.size() : HP_ERR_ARG; }

extern "C" int hp_net_feature_map(const hp_net* net, int index, const float** d_ptr, int* h, int* w, int* c) {
  HP_REQUIRE(net && net->finalized, "hp_net_feature_map: network not finalized");
  HP_REQUIRE(index >= 0 && index < (int)net->feature_maps.size(), "hp_net_feature_map: no such feature map");
  const auto& f = net->feature_maps[index];
  if (d_ptr) *d_ptr = (const float*)net->bufs[f.buf].p;
  if (h) *h = f.H;
  if (w) *w = f.W;
  if (c) *c = f.C;
  return HP_OK;
}

extern "C" int hp_net_copy_feature_map(const hp_net* net, int index, int batch, float* d_dst, void* stream) {
  HP_REQUIRE(net && net->finalized && d_dst, "hp_net_copy_feature_map: bad argument");
  HP_REQUIRE(index >= 0 && index < (int)net->feature_maps.size(), "hp_net_copy_feature_map: no such feature map");
  HP_REQUIRE(batch >= 0 && batch <= net->max_batch, "hp_net_copy_feature_map: batch exceeds max_batch");
  const auto& f = net->feature_maps[index];
  HP_CHECK_HIP(hipMemcpyAsync(d_dst, net->bufs[f.buf].p, (size_t)batch * f.H * f.W * f.C * sizeof(float), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return HP_OK;
}

extern "C" int hp_net_n_ops(const hp_net* net) { return net && net->finalized ? (int)net->ops.size() : HP_ERR_ARG; }

extern "C" int hp_net_op_info(const hp_net* net, int index, hp_op_info* info) {
  HP_REQUIRE(net && net->finalized && info, "hp_net_op_info: network not finalized / null info");
  HP_REQUIRE(index >= 0 && index < (int)net->ops.size(), "hp_net_op_info: no such op");
  const Op& op = net->ops[index];
  hp_op_info r{};
  static_assert(OP_CONV == HP_OP_CONV && OP_MAXPOOL == HP_OP_MAXPOOL && OP_HEAD == HP_OP_HEAD && OP_DW == HP_OP_DWCONV &&
                OP_SE == HP_OP_SE && OP_RESIZE == HP_OP_RESIZE, "OpKind and HP_OP_* share their values");
  r.kind = (int)op.kind;
  r.in_slot = op.in_buf; r.out_slot = op.out_buf; r.res_slot = -1;
  r.H = op.H; r.W = op.W; r.Cin = r.Cout = op.C; r.Ho = op.Ho; r.Wo = op.Wo;
  r.elem_bytes = net->precision == HP_PRECISION_F16 ? 2 : 4;
  std::string name;
  if (op.kind == OP_CONV) {
    const ConvLayer& L = *net->convs[op.conv];
    name = L.wname;
    r.k = L.kh; r.stride = L.stride; r.pad = L.pad; r.act = L.relu;
    r.H = L.H; r.W = L.W; r.Cin = L.cin_real; r.Ho = L.Ho; r.Wo = L.Wo; r.Cout = L.cout;
    r.prologue = L.bn_before.empty() ? 0 : 1;
    r.in_slot = L.in_buf; r.res_slot = L.res_buf; r.out_slot = L.out_buf;
  } else if (op.kind == OP_DW) {
    const DwLayer& D = *net->dws[op.conv];
    name = D.wname;
    r.k = D.k; r.stride = D.stride; r.pad = D.pad; r.act = HP_ACT_SWISH;
    r.H = D.H; r.W = D.W; r.Cin = r.Cout = D.C; r.Ho = D.Ho; r.Wo = D.Wo;
    r.in_slot = D.in_buf; r.out_slot = D.out_buf;
  } else if (op.kind == OP_SE) {
    const SeLayer& S = *net->ses[op.conv];
    name = S.prefix;
    r.H = S.HW; r.W = 1; r.Cin = S.C; r.Cout = S.Cse; r.in_slot = S.in_buf; r.out_slot = -1;
  } else if (op.kind == OP_MAXPOOL) {
    r.k = 3; r.stride = 2; r.pad = 1;
  } else if (op.kind == OP_HEAD) {
    r.out_slot = -1; r.Cout = net->n_features;
  }
  std::strncpy(r.name, name.c_str(), sizeof(r.name) - 1);
  r.path = net->op_path[index];
  r.materialised = net->op_mat[index];
  *info = r;
  return HP_OK;
}

extern "C" int hp_net_set_taps(hp_net* net, int n, const int* op_index, void* const* d_dst) {
  HP_REQUIRE(net && net->finalized && n >= 0 && (n == 0 || (op_index && d_dst)), "hp_net_set_taps: network not finalized / bad argument");
  std::vector<void*> taps(n ? net->ops.size() : 0, nullptr);
  for (int i = 0; i < n; ++i) {
    HP_REQUIRE(op_index[i] >= 0 && op_index[i] < (int)net->ops.size(), "hp_net_set_taps: no such op");
    const OpKind k = net->ops[op_index[i]].kind;
    HP_REQUIRE(k != OP_HEAD && k != OP_SE, "hp_net_set_taps: the head and squeeze-excitation ops have no output map");
    HP_REQUIRE(d_dst[i], "hp_net_set_taps: null destination");
    taps[op_index[i]] = d_dst[i];
  }
  net->taps.swap(taps);
  return HP_OK;
}

extern "C" int hp_detector_preprocess(const float* d_images, int n, int h, int w, const float* h_mean3, const float* h_std3,
                                      float* d_x_nhwc4, void* stream) {
  HP_REQUIRE(d_images && d_x_nhwc4 && h_mean3 && h_std3 && n >= 0 && h > 0 && w > 0, "hp_detector_preprocess: bad argument");
  if (n == 0) return HP_OK;
  return launch_normalize_nhwc4(d_images, d_x_nhwc4, n, h, w, h_mean3, h_std3, (hipStream_t)stream);
}

extern "C" int hp_detector_preprocess_resize(const float* d_images, int n, int h_in, int w_in, int h_out, int w_out, int h_pad,
                                             int w_pad, const float* h_mean3, const float* h_std3, float* d_x_nhwc4,
                                             void* stream) {
  HP_REQUIRE(d_images && d_x_nhwc4 && h_mean3 && h_std3 && n >= 0 && h_in > 0 && w_in > 0 && h_out > 0 && w_out > 0 &&
                 h_pad >= h_out && w_pad >= w_out, "hp_detector_preprocess_resize: bad argument");
  if (n == 0) return HP_OK;
  return launch_normalize_resize_nhwc4(d_images, d_x_nhwc4, n, h_in, w_in, h_out, w_out, h_pad, w_pad, h_mean3, h_std3,
                                       (hipStream_t)stream);
}

extern "C" int hp_net_input_channels_f16(const hp_net* net) {
  return net && net->finalized && net->precision == HP_PRECISION_F16 ? net->convs[0]->cin16 : HP_ERR_ARG;
}

extern "C" int hp_net_forward_f16in(hp_net* net, const void* d_x16, int batch, float* d_pose, float* d_logits,
                                    float* d_features, void* stream) {
  HP_REQUIRE(net && net->finalized, "hp_net_forward_f16in: network not finalized");
  HP_REQUIRE(net->precision == HP_PRECISION_F16, "hp_net_forward_f16in: the network was not planned in fp16");
  HP_REQUIRE(batch >= 0, "hp_net_forward_f16in: negative batch");
  if (batch == 0) return HP_OK;
  HP_REQUIRE(d_x16, "hp_net_forward_f16in: null input");
  HP_REQUIRE(!d_pose || net->pose_dim > 0, "hp_net_forward_f16in: network has no pose head");
  HP_REQUIRE(!d_logits || net->n_logits > 0, "hp_net_forward_f16in: network has no logits head");
  hipStream_t st = (hipStream_t)stream;
  int rc_t = taps_allowed(net, st);
  if (rc_t) return rc_t;
  const size_t in_stride = (size_t)net->h * net->w * net->convs[0]->cin16 * sizeof(_Float16);
  for (int b0 = 0; b0 < batch; b0 += net->max_batch) {
    const int nb = batch - b0 < net->max_batch ? batch - b0 : net->max_batch;
    int rc = forward_chunk(net, nullptr, (const char*)d_x16 + (size_t)b0 * in_stride, b0, nb,
                           d_pose ? d_pose + (size_t)b0 * net->pose_dim : nullptr,
                           d_logits ? d_logits + (size_t)b0 * net->n_logits : nullptr,
                           d_features ? d_features + (size_t)b0 * net->n_features : nullptr, st);
    if (rc) return rc;
  }
  return HP_OK;
}

extern "C" int hp_net_profile_collect(hp_net* net, double* conv_ms, int64_t* n_launches, double* conv_flops,
                                      double* mfma_flops) {
  HP_REQUIRE(net, "hp_net_profile_collect: null net");
  double ms_total = 0.0, fl = 0.0, mfl = 0.0;
  const bool verbose = dbg(DBG_PROFILE_LAYERS) != 0;
  std::vector<double> lms(net->convs.size(), 0.0), lfl(net->convs.size(), 0.0);
  std::vector<int> lcnt(net->convs.size(), 0);
  for (auto& p : net->ev_pending) {
    HP_CHECK_HIP(hipEventSynchronize(p.e1));
    float ms = 0.f;
    HP_CHECK_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
    ms_total += ms;
    fl += p.flops;
    mfl += p.mfma_flops;
    if (p.conv >= 0) { lms[p.conv] += ms; lfl[p.conv] += p.flops; lcnt[p.conv]++; }
    net->ev_pool.push_back(p);
  }
  if (verbose) {  // per-layer table (stderr): which convolution shapes lag the roofline
    for (size_t i = 0; i < net->convs.size(); ++i) {
      if (!lcnt[i]) continue;
      const ConvLayer& L = *net->convs[i];
      std::fprintf(stderr, "[hp conv] %-38s %dx%d s%d %4d->%4d @%3dx%3d  K=%5d  %8.1f us  %6.1f TFLOP/s\n",
                   L.wname.c_str(), L.kh, L.kw, L.stride, L.cin_real, L.cout, L.Ho, L.Wo, L.Kpad,
                   1e3 * lms[i] / lcnt[i], lfl[i] / (lms[i] * 1e-3) / 1e12);
    }
  }
  if (conv_ms) *conv_ms = ms_total;
  int64_t nl = 0;
  for (auto& p : net->ev_pending) nl += p.n;
  if (n_launches) *n_launches = nl;
  if (conv_flops) *conv_flops = fl;
  if (mfma_flops) *mfma_flops = mfl;
  net->ev_pending.clear();
  return HP_OK;
}

extern "C" double hp_net_flops_per_sample(const hp_net* net) { return net ? net->flops_per_sample : 0.0; }

// ---- profiling across several networks / streams: absolute positions of the timed stretches -------------
namespace { hipEvent_t g_prof_ref = nullptr; }

extern "C" int hp_profile_mark_reference(void* stream) {
  if (!g_prof_ref) HP_CHECK_HIP(hipEventCreate(&g_prof_ref));
  HP_CHECK_HIP(hipEventRecord(g_prof_ref, (hipStream_t)stream));
  return HP_OK;
}

extern "C" int hp_net_profile_intervals(hp_net* net, double* t0_ms, double* t1_ms, int cap) {
  HP_REQUIRE(net, "hp_net_profile_intervals: null net");
  HP_REQUIRE(g_prof_ref, "hp_net_profile_intervals: hp_profile_mark_reference has not been called");
  HP_REQUIRE(cap >= 0 && (cap == 0 || (t0_ms && t1_ms)), "hp_net_profile_intervals: bad buffers");
  int n = 0;
  for (auto& p : net->ev_pending) {
    if (n < cap) {
      HP_CHECK_HIP(hipEventSynchronize(p.e1));
      float a = 0.f, b = 0.f;
      HP_CHECK_HIP(hipEventElapsedTime(&a, g_prof_ref, p.e0));
      HP_CHECK_HIP(hipEventElapsedTime(&b, g_prof_ref, p.e1));
      t0_ms[n] = a; t1_ms[n] = b;
    }
    ++n;
  }
  return n;
}

extern "C" int hp_net_set_conv_algo(hp_net* net, int algo) {
  HP_REQUIRE(net, "hp_net_set_conv_algo: null net");
  HP_REQUIRE(algo >= -1 && algo <= HP_CONV_ALGO_SPLIT, "hp_net_set_conv_algo: unknown algorithm");
  net->algo = algo;
  return HP_OK;
}

extern "C" int hp_net_set_act_scale(hp_net* net, int enabled) {
  HP_REQUIRE(net, "hp_net_set_act_scale: null net");
  net->act_scale = enabled != 0;
  return HP_OK;
}

extern "C" int hp_net_set_tail_split(hp_net* net, int enabled) {
  HP_REQUIRE(net, "hp_net_set_tail_split: null net");
  net->tail_split = enabled != 0;
  return HP_OK;
}

extern "C" int hp_net_status(hp_net* net, void* stream, int* flags) {
  HP_REQUIRE(net && flags, "hp_net_status: null argument");
  *flags = 0;
  if (!net->finalized) return HP_OK;
  HP_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  const bool f16 = net->precision == HP_PRECISION_F16;
  if (*(volatile unsigned*)net->h_status) {
    *flags |= HP_STATUS_NONFINITE;
    // a re-run of the same inputs takes the exact-fp32 kernels; an fp16 network has none: the caller repeats the stage on
    // an HP_PRECISION_F32 network of the same parameters (happypose_amd.ops.Net does)
    if (!f16) net->exact_only = true;
    *(volatile unsigned*)net->h_status = 0u;
  }
  if (net->exact_only && !f16) *flags |= HP_STATUS_EXACT_ONLY;
  return HP_OK;
}

extern "C" int hp_net_force_exact(hp_net* net, int enabled) {
  HP_REQUIRE(net, "hp_net_force_exact: null net");
  net->exact_only = enabled != 0;
  return HP_OK;
}

extern "C" int hp_net_set_profiling(hp_net* net, int enabled) {
  HP_REQUIRE(net, "hp_net_set_profiling: null net");
  net->profiling = enabled != 0;
  return HP_OK;
}


// ---- single-layer entries for the kernel parity tests ------------------------------------
namespace {

// grow-only per-process scratch: the planner packs and transforms weights once at load time, these test entries on every call
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  int grow(size_t need) {
    if (bytes >= need) return HP_OK;
    if (p) (void)hipFree(p);
    p = nullptr; bytes = 0;
    HP_CHECK_HIP(hipMalloc(&p, need));
    bytes = need;
    return HP_OK;
  }
};

// The gather table of a single-layer call: [Kpad / gran + extra] entries {offset, kh, kw, channel} over K in steps of `gran`
// elements (4 floats, 8 halves), kh < 0 marking K padding.  It lives until the stream has consumed it: allocate, async copy,
// free after sync is avoided by keeping a small per-process cache keyed on the geometry.
struct LutCache {
  std::map<std::string, int4*> map;
  std::mutex mutex;
  int get(int gran, int extra, int w, int cin, int kh, int kw, int Kreal, int Kpad, int4** d_lut) {  // with `mutex` held
    int cur_dev = 0;
    HP_CHECK_HIP(hipGetDevice(&cur_dev));
    const std::string key = std::to_string(cur_dev) + "_" + std::to_string(w) + "_" + std::to_string(cin) + "_" + std::to_string(kh);
    auto it = map.find(key);
    if (it != map.end()) { *d_lut = it->second; return HP_OK; }
    std::vector<int4> lut(Kpad / gran + extra, make_int4(0, -1, 0, 0));
    for (int q = 0; q < Kreal / gran; ++q) {
      const int k = gran * q, seg = k / cin, ch = k % cin, y = seg / kw, x = seg % kw;
      lut[q] = make_int4((y * w + x) * cin + ch, y, x, ch);
    }
    HP_CHECK_HIP(hipMalloc((void**)d_lut, lut.size() * sizeof(int4)));
    HP_CHECK_HIP(hipMemcpy(*d_lut, lut.data(), lut.size() * sizeof(int4), hipMemcpyHostToDevice));
    map[key] = *d_lut;
    return HP_OK;
  }
};

}  // namespace

extern "C" int hp_conv2d_nhwc(const float* d_x, int n, int h, int w, int cin, const float* d_w, int cout,
                              int kh, int kw, int stride, int pad, const float* d_bias,
                              const float* d_residual, const float* d_pre_scale,
                              const float* d_pre_shift, int relu, float* d_y, void* stream) {
  HP_REQUIRE(d_x && d_w && d_y, "hp_conv2d_nhwc: null pointer");
  HP_REQUIRE(cin % 4 == 0 && cin > 0, "hp_conv2d_nhwc: cin must be a multiple of 4");
  HP_REQUIRE(cout % 4 == 0 && cout > 0, "hp_conv2d_nhwc: cout must be a multiple of 4");
  HP_REQUIRE(kh == kw && kh >= 1 && (stride == 1 || stride == 2) && pad >= 0, "hp_conv2d_nhwc: unsupported geometry");
  HP_REQUIRE(d_pre_scale || !d_pre_shift, "hp_conv2d_nhwc: pre_shift without pre_scale");
  HP_REQUIRE(relu >= HP_ACT_NONE && relu <= HP_ACT_SWISH, "hp_conv2d_nhwc: unknown activation");
  int rc = conv_setup_once();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Kreal = kh * kw * cin, Kpad = (Kreal + 31) / 32 * 32;
  // weights / bias padded to whole 64-wide tiles and to a multiple of 32 in K
  const int cout_pad = (cout + 63) / 64 * 64;
  if (cout_pad != cout || Kpad != Kreal) {
    static Scratch wp;
    const size_t need = (size_t)cout_pad * Kpad + cout_pad;
    if ((rc = wp.grow(need * sizeof(float)))) return rc;
    float* d_wp = (float*)wp.p;
    HP_CHECK_HIP(hipMemsetAsync(d_wp, 0, need * sizeof(float), st));
    HP_CHECK_HIP(hipMemcpy2DAsync(d_wp, (size_t)Kpad * 4, d_w, (size_t)Kreal * 4, (size_t)Kreal * 4, cout,
                                  hipMemcpyDeviceToDevice, st));
    if (d_bias) HP_CHECK_HIP(hipMemcpyAsync(d_wp + (size_t)cout_pad * Kpad, d_bias, (size_t)cout * 4, hipMemcpyDeviceToDevice, st));
    d_w = d_wp;
    if (d_bias) d_bias = d_wp + (size_t)cout_pad * Kpad;
  }
  static LutCache cache;
  std::lock_guard<std::mutex> cache_lock(cache.mutex);
  int4* d_lut = nullptr;
  if ((rc = cache.get(4, 16, w, cin, kh, kw, Kreal, Kpad, &d_lut))) return rc;  // + 16: the kernel prefetches two K-tiles ahead
  ConvArgs a{};
  a.x = d_x; a.w = d_w; a.bias = d_bias; a.residual = d_residual; a.pre_scale = d_pre_scale;
  a.pre_shift = d_pre_shift; a.lut = d_lut; a.y = d_y;
  a.H = h; a.W = w; a.Cin = cin; a.Ho = (h + 2 * pad - kh) / stride + 1; a.Wo = (w + 2 * pad - kw) / stride + 1;
  a.Cout = cout; a.stride = stride; a.pad = pad; a.Kpad = Kpad; a.ktiles = Kpad / 32; a.relu = relu;
  a.M = (int64_t)n * a.Ho * a.Wo;
  a.algo = conv_layer_algo();
  // the site of a layer without neighbours, its weight sets made on demand
  ConvSite s;
  s.H = h; s.W = w; s.Cin = s.cin_real = cin; s.Ho = a.Ho; s.Wo = a.Wo; s.Cout = cout; s.kh = kh; s.kw = kw; s.stride = stride; s.pad = pad;
  s.act = relu; s.prologue = d_pre_scale && d_pre_shift; s.se_gated = d_pre_scale && !d_pre_shift;
  s.residual = d_residual != nullptr; s.bias = d_bias != nullptr; s.cout_pad = cout_pad; s.Kpad = Kpad;
  s.isplit_beside_split = s.wino_classic_only = true;
  const WeightSets sets = conv_weight_sets(s);
  s.has_split = sets.split; s.has_isplit = sets.isplit; s.has_wino = sets.wino;
  s.algo = a.algo; s.batch = n;
  const ConvChoice ch = choose_conv(s);
  static Scratch ws[W_STEM7];  // one per transformed set
  switch (ch.path) {
    case HP_PATH_SPLIT3X3:
      if ((rc = ws[W_SPLIT].grow(conv_split_weight_bytes(cout, cin)))) return rc;
      if ((rc = conv_split_transform_weights(d_w, ws[W_SPLIT].p, cout, cin, Kpad, stride, st))) return rc;
      a.w = (const float*)ws[W_SPLIT].p;
      return launch_conv_split(a, st);
    case HP_PATH_WINOGRAD:
      if ((rc = ws[W_WINO].grow(conv_wino_weight_floats(cout, cin) * sizeof(float)))) return rc;
      if ((rc = conv_wino_transform_weights(d_w, (float*)ws[W_WINO].p, cout, cin, Kpad, st))) return rc;
      a.w = (const float*)ws[W_WINO].p;
      return launch_conv_wino(a, st);
    case HP_PATH_IGEMM_SPLIT:
      if ((rc = ws[W_ISPLIT].grow(conv_igemm_split_weight_bytes(cout_pad, Kpad)))) return rc;
      if ((rc = conv_igemm_split_transform_weights(d_w, ws[W_ISPLIT].p, cout_pad, Kpad, st))) return rc;
      a.w = (const float*)ws[W_ISPLIT].p;
      return launch_conv_igemm_split(a, ch.variant, st);
    case HP_PATH_PATCH: return launch_conv_patch(a, ch.variant, st);
    default: return launch_conv(a, ch.variant, st);
  }
}

// ---- single-layer entry of the fp16 kernel for the parity tests (all tensors fp16 except bias) ----
extern "C" int hp_conv2d_nhwc_f16(const void* d_x, int n, int h, int w, int cin, const void* d_w, int cout, int kh,
                                  int kw, int stride, int pad, const float* d_bias, const void* d_residual,
                                  const void* d_pre_scale, const void* d_pre_shift, int relu, void* d_y,
                                  void* stream) {
  HP_REQUIRE(d_x && d_w && d_y, "hp_conv2d_nhwc_f16: null pointer");
  HP_REQUIRE(cin % 8 == 0 && cin > 0, "hp_conv2d_nhwc_f16: cin must be a multiple of 8");
  HP_REQUIRE(cout % 64 == 0 && cout > 0, "hp_conv2d_nhwc_f16: cout must be a multiple of 64");
  HP_REQUIRE(kh == kw && kh >= 1 && (stride == 1 || stride == 2) && pad >= 0, "hp_conv2d_nhwc_f16: unsupported geometry");
  HP_REQUIRE((d_pre_scale == nullptr) == (d_pre_shift == nullptr), "hp_conv2d_nhwc_f16: pre_scale/pre_shift must come together");
  const int Kreal = kh * kw * cin, Kpad = (Kreal + 63) / 64 * 64;
  HP_REQUIRE(Kreal == Kpad, "hp_conv2d_nhwc_f16: kh*kw*cin must be a multiple of 64 (weights are [cout][kh][kw][cin])");
  static LutCache cache;
  std::lock_guard<std::mutex> cache_lock(cache.mutex);
  int4* d_lut = nullptr;
  int rc = cache.get(8, 0, w, cin, kh, kw, Kreal, Kpad, &d_lut);
  if (rc) return rc;
  ConvArgsH a{};
  a.x = (const _Float16*)d_x; a.w = (const _Float16*)d_w; a.bias = d_bias; a.residual = (const _Float16*)d_residual;
  a.pre_scale = (const _Float16*)d_pre_scale; a.pre_shift = (const _Float16*)d_pre_shift; a.lut = d_lut;
  a.y = (_Float16*)d_y;
  a.H = h; a.W = w; a.Cin = cin; a.Ho = (h + 2 * pad - kh) / stride + 1; a.Wo = (w + 2 * pad - kw) / stride + 1;
  a.Cout = cout; a.stride = stride; a.pad = pad; a.Kpad = Kpad; a.ktiles = Kpad / 64; a.relu = relu;
  a.kh = kh; a.kw = kw;
  a.M = (int64_t)n * a.Ho * a.Wo;
  a.x_bytes = (int64_t)n * h * w * cin * 2;
  a.w_bytes = (int64_t)cout * Kpad * 2;
  return launch_conv_f16(a, (hipStream_t)stream);
}
