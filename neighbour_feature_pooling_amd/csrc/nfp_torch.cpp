// nfp_torch.cpp — C++ autograd nodes over the C ABI of libnfp_hip.so (include/nfp.h).
//
// The reference's NFP is a chain of ATen ops whose autograd graph PyTorch builds (nfp.py:132-159); here one
// forward and one backward kernel stand for it, and these torch::autograd::Function classes are the graph
// nodes.  They do what functional.py's Python autograd.Functions do — allocate out / saved / grad_x, take torch's
// current stream, call nfp_forward / nfp_backward (nfp_pool_* / nfp_gap_* / nfp_valid_* / nfp_valid_abs_*) — without the Python
// interpreter on the launch path: eager host cost per forward + backward drops from ~75 us to the autograd
// engine's own (scripts/host_overhead.py).  No device code in this file; plain pointers go across the ABI.
//
// Built by neighbour_feature_pooling_amd/build.py::build_torch_ext (g++ against libtorch + libnfp_hip.so);
// optional: functional.py falls back to its Python nodes when the module is absent.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include "../../include/nfp.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void check(int rc) {
  if (rc == NFP_OK) return;
  // the Python binding maps the prefix back onto NfpUnsupported / NfpError
  TORCH_CHECK(false, rc == NFP_E_UNSUPPORTED ? "libnfp_hip unsupported: " : "libnfp_hip error: ", nfp_last_error());
}

void* stream_of(const Tensor& x) { return (void*)c10::hip::getCurrentHIPStream(x.device().index()).stream(); }

Tensor empty_like_layout(const Tensor& x, bool nhwc) {
  return torch::empty(x.sizes(), x.options().memory_format(nhwc ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous));
}

// desc: CPU uint8 tensor holding one nfp_desc (the plan's descriptor; functional.py keeps it alive)
const nfp_desc* desc_of(const Tensor& desc) {
  TORCH_CHECK(desc.device().is_cpu() && desc.scalar_type() == torch::kUInt8 && desc.numel() == (int64_t)sizeof(nfp_desc),
              "descriptor tensor must be ", sizeof(nfp_desc), " bytes on the CPU");
  return (const nfp_desc*)desc.data_ptr();
}

struct NfpNode : torch::autograd::Function<NfpNode> {
  static Tensor forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
    c10::DeviceGuard guard(x.device());
    const nfp_desc* d = desc_of(desc);
    // (d->map_f32: bf16 x with float32 maps — the torch.autocast call, include/nfp.h)
    Tensor out = torch::empty(oshape, (d->map_f32 ? x.options().dtype(torch::kFloat32) : x.options()).memory_format(at::MemoryFormat::Contiguous));
    Tensor saved = torch::empty({ns}, x.options().dtype(torch::kFloat32).memory_format(at::MemoryFormat::Contiguous));
    check(nfp_forward(d, x.data_ptr(), out.data_ptr(), ns > 0 ? saved.data_ptr<float>() : nullptr, stream_of(x)));
    ctx->save_for_backward({x, out, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &out = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    Tensor go = grads[0].contiguous();
    if (go.scalar_type() != out.scalar_type()) go = go.to(out.scalar_type());   // (grad_out in the maps' type: x's, or float32)
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_backward(desc_of(desc), x.data_ptr(), go.data_ptr(), out.data_ptr(),
                       saved.numel() ? saved.data_ptr<float>() : nullptr, gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// want_gap: GAP(x) is part of the result (NFP_Pooling.py:27); false: the pooled NFP maps alone (texture_pooling.py:251-252)
// — an empty tensor stands in for it.  need_grad: a backward will follow — only then are the maps themselves stored.
struct NfpPoolNode : torch::autograd::Function<NfpPoolNode> {
  static variable_list forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns,
                               bool nhwc, bool want_gap, bool need_grad) {
    c10::DeviceGuard guard(x.device());
    const nfp_desc* d = desc_of(desc);
    const auto f32 = x.options().dtype(torch::kFloat32).memory_format(at::MemoryFormat::Contiguous);
    Tensor gap = torch::empty({want_gap ? oshape[0] : 0, x.size(1)}, f32), nfpm = torch::empty({oshape[0], oshape[1]}, f32);
    Tensor omap = need_grad ? torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous))
                            : torch::empty({0}, x.options());
    Tensor saved = torch::empty({ns}, f32);
    check(nfp_pool_forward(d, x.data_ptr(), want_gap ? gap.data_ptr<float>() : nullptr, nfpm.data_ptr<float>(),
                           need_grad ? omap.data_ptr() : nullptr, ns > 0 ? saved.data_ptr<float>() : nullptr, stream_of(x)));
    ctx->save_for_backward({x, omap, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    ctx->saved_data["want_gap"] = want_gap;
    return {gap, nfpm};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &omap = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    const auto f32 = x.options().dtype(torch::kFloat32);
    // a pooled output that took no part in the loss arrives undefined: its gradient is zero
    // (grad_gap = NULL: GAP(x) was not produced, or took no part in the loss — no adjoint of the mean, include/nfp.h)
    const bool has_gap = ctx->saved_data["want_gap"].toBool() && grads[0].defined();
    Tensor ggap = has_gap ? grads[0].contiguous().to(torch::kFloat32) : Tensor();
    Tensor gnfp = grads[1].defined() ? grads[1].contiguous().to(torch::kFloat32)
                                     : torch::zeros({omap.size(0), omap.size(1)}, f32);
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_pool_backward(desc_of(desc), x.data_ptr(), has_gap ? ggap.data_ptr<float>() : nullptr, gnfp.data_ptr<float>(),
                            omap.data_ptr(), saved.numel() ? saved.data_ptr<float>() : nullptr, gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// GAP(x) beside the full maps (nfp_gap_forward / nfp_gap_backward): one radius, or radii (1, 2) together (desc.inner_R).
// An output that took no part in the loss arrives undefined (set_materialize_grads(false)): gap undefined -> grad_gap =
// NULL, maps undefined -> a zero map, both undefined -> no launch.
struct NfpGapNode : torch::autograd::Function<NfpGapNode> {
  static variable_list forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
    c10::DeviceGuard guard(x.device());
    const nfp_desc* d = desc_of(desc);
    const auto f32 = x.options().dtype(torch::kFloat32).memory_format(at::MemoryFormat::Contiguous);
    Tensor gap = torch::empty({x.size(0), x.size(1)}, f32);
    Tensor maps = torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous));
    Tensor saved = torch::empty({ns > 0 ? ns : 1}, f32);
    check(nfp_gap_forward(d, x.data_ptr(), gap.data_ptr<float>(), maps.data_ptr(), saved.data_ptr<float>(), saved.numel(),
                          stream_of(x)));
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({x, maps, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return {gap, maps};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    if (!grads[0].defined() && !grads[1].defined()) return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &maps = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    const bool has_gap = grads[0].defined();
    Tensor ggap = has_gap ? grads[0].contiguous().to(torch::kFloat32) : Tensor();
    Tensor go = grads[1].defined() ? grads[1].contiguous() : torch::zeros_like(maps);
    if (go.scalar_type() != x.scalar_type()) go = go.to(x.scalar_type());
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_gap_backward(desc_of(desc), x.data_ptr(), has_gap ? ggap.data_ptr<float>() : nullptr, go.data_ptr(),
                           maps.data_ptr(), saved.data_ptr<float>(), saved.numel(), gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// The maps of an unpadded layer on the valid-map kernels (nfp_valid_forward / nfp_valid_backward): NfpNode with the length
// convention of those calls.  ns = 0: no backward will follow (nothing is saved, `saved` goes over as NULL).
struct NfpValidNode : torch::autograd::Function<NfpValidNode> {
  static Tensor forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
    c10::DeviceGuard guard(x.device());
    Tensor out = torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous));
    Tensor saved = torch::empty({ns}, x.options().dtype(torch::kFloat32).memory_format(at::MemoryFormat::Contiguous));
    check(nfp_valid_forward(desc_of(desc), x.data_ptr(), out.data_ptr(), ns > 0 ? saved.data_ptr<float>() : nullptr, ns,
                            stream_of(x)));
    ctx->save_for_backward({x, out, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &out = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    Tensor go = grads[0].contiguous();
    if (go.scalar_type() != out.scalar_type()) go = go.to(out.scalar_type());
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_valid_backward(desc_of(desc), x.data_ptr(), go.data_ptr(), out.data_ptr(),
                             saved.numel() ? saved.data_ptr<float>() : nullptr, saved.numel(), gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// ... and their L1 family (nfp_valid_abs_forward / nfp_valid_abs_backward: Norm p = 1 on the difference weights, EMD): the
// backward reads x and grad_out alone, so x is all the node saves and the maps may be modified in place by the caller.
struct NfpValidAbsNode : torch::autograd::Function<NfpValidAbsNode> {
  static Tensor forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, bool nhwc, bool need_grad) {
    c10::DeviceGuard guard(x.device());
    Tensor out = torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous));
    check(nfp_valid_abs_forward(desc_of(desc), x.data_ptr(), out.data_ptr(), stream_of(x)));
    if (need_grad) ctx->save_for_backward({x, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &desc = sv[1];
    c10::DeviceGuard guard(x.device());
    Tensor go = grads[0].contiguous();
    if (go.scalar_type() != x.scalar_type()) go = go.to(x.scalar_type());
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_valid_abs_backward(desc_of(desc), x.data_ptr(), go.data_ptr(), gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor nfp_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return NfpNode::apply(x, desc, oshape, ns, nhwc);
}
Tensor nfp_valid_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return NfpValidNode::apply(x, desc, oshape, ns, nhwc);
}
Tensor nfp_valid_abs_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, bool nhwc, bool need_grad) {
  return NfpValidAbsNode::apply(x, desc, oshape, nhwc, need_grad);
}
std::vector<Tensor> nfp_pool_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc, bool want_gap,
                                   bool need_grad) {
  return NfpPoolNode::apply(x, desc, oshape, ns, nhwc, want_gap, need_grad);
}

std::vector<Tensor> nfp_gap_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return NfpGapNode::apply(x, desc, oshape, ns, nhwc);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("nfp_apply", &nfp_apply, "NFPPooling.forward as one autograd node (nfp_forward / nfp_backward)");
  m.def("nfp_pool_apply", &nfp_pool_apply, "the fused nfp_pooling tail as one autograd node (nfp_pool_forward / _backward)");
  m.def("nfp_gap_apply", &nfp_gap_apply, "GAP(x) beside the full maps as one autograd node (nfp_gap_forward / _backward)");
  m.def("nfp_valid_apply", &nfp_valid_apply, "an unpadded layer's maps as one autograd node (nfp_valid_forward / _backward)");
  m.def("nfp_valid_abs_apply", &nfp_valid_abs_apply,
        "an unpadded L1 layer's maps as one autograd node that saves x alone (nfp_valid_abs_forward / _backward)");
  m.attr("desc_bytes") = (int64_t)sizeof(nfp_desc);
}
