// JetVector elementwise + geometry ops.  Each op's arithmetic is written once,
// as a per-item body usable on host and device; forEachItem() runs a body
// over all items as one grid-stride HIP kernel (gfx950) or as an OpenMP loop.
// The bodies are templates over the op and the operand kinds.
// Reference anchor: src/operator/jet_vector_math_impl.cu (39 hand-written
// kernels) and src/operator/jet_vector_math_impl.cpp (host backend).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "../jet.hpp"  // MEGBA_HD
#include "jetvector.hpp"

namespace megba {

#define JV_HIP_CHECK(expr)                                                   \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    MEGBA_CHECK(_e == hipSuccess,                                            \
                std::string("HIP error: ") + hipGetErrorString(_e));         \
  } while (0)

// Caching device allocator for JetVector temporaries -- the MemoryPool
// equivalent (reference C4, src/resource/memory_pool.cu): residual
// expressions allocate/free same-sized blocks every forward, so freed blocks
// go to a size-keyed free list instead of hipFree.  No LIFO discipline is
// needed (the reference threw on out-of-order frees, memory_pool.cu:169).
namespace {
std::mutex gPoolMu;
std::unordered_map<size_t, std::vector<void*>> gPool;

void* poolAlloc(size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(gPoolMu);
    auto it = gPool.find(bytes);
    if (it != gPool.end() && !it->second.empty()) {
      void* p = it->second.back();
      it->second.pop_back();
      return p;
    }
  }
  void* p = nullptr;
  JV_HIP_CHECK(hipMalloc(&p, bytes));
  return p;
}

void poolFree(void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(gPoolMu);
  gPool[bytes].push_back(p);
}
}  // namespace

// (DeviceBuf dtor defined after the pool so it can return blocks to it.)
void jvPoolTrim() {
  std::lock_guard<std::mutex> lk(gPoolMu);
  for (auto& kv : gPool)
    for (void* p : kv.second) (void)hipFree(p);
  gPool.clear();
}

template <typename T>
DeviceBuf<T>::~DeviceBuf() {
  if (!ptr || !owned) return;
  if (onGpu)
    poolFree(ptr, (n > 0 ? n : 1) * sizeof(T));
  else
    free(ptr);
}
template struct DeviceBuf<double>;
template struct DeviceBuf<float>;

template <typename T>
JetVec<T> jvView(T* ptr, int64_t nItem, int N, int gradPos, bool onGpu) {
  JetVec<T> v;
  v.nItem = nItem;
  v.N = N;
  v.gradPos = gradPos;
  v.onGpu = onGpu;
  v.value = std::make_shared<DeviceBuf<T>>();
  v.value->ptr = ptr;
  v.value->n = nItem;
  v.value->onGpu = onGpu;
  v.value->owned = false;
  return v;
}
template JetVec<double> jvView<double>(double*, int64_t, int, int, bool);
template JetVec<float> jvView<float>(float*, int64_t, int, int, bool);

namespace {

template <typename T>
std::shared_ptr<DeviceBuf<T>> makeBuf(int64_t n, bool onGpu) {
  auto b = std::make_shared<DeviceBuf<T>>();
  b->n = n;
  b->onGpu = onGpu;
  if (onGpu) {
    b->ptr = (T*)poolAlloc((n > 0 ? n : 1) * sizeof(T));
  } else {
    b->ptr = (T*)malloc((n > 0 ? n : 1) * sizeof(T));
    MEGBA_CHECK(b->ptr, "malloc failed");
  }
  return b;
}

// Host memory <-> a JetVector's backend memory.
template <typename T>
void copyIn(bool onGpu, T* dst, const T* host, int64_t count) {
  if (onGpu)
    JV_HIP_CHECK(hipMemcpy(dst, host, count * sizeof(T), hipMemcpyHostToDevice));
  else
    std::memcpy(dst, host, count * sizeof(T));
}
template <typename T>
void copyOut(bool onGpu, T* host, const T* src, int64_t count) {
  if (onGpu)
    JV_HIP_CHECK(hipMemcpy(host, src, count * sizeof(T), hipMemcpyDeviceToHost));
  else
    std::memcpy(host, src, count * sizeof(T));
}

// Dense output shaped like `ref`.
template <typename T>
JetVec<T> denseLike(const JetVec<T>& ref) {
  JetVec<T> out;
  out.nItem = ref.nItem;
  out.N = ref.N;
  out.onGpu = ref.onGpu;
  out.value = makeBuf<T>(out.nItem, out.onGpu);
  out.grad = makeBuf<T>((int64_t)out.N * out.nItem, out.onGpu);
  return out;
}

// Dense output of a binary op, after checking that the operands agree.
template <typename T>
JetVec<T> denseLike(const JetVec<T>& a, const JetVec<T>& b) {
  const JetVec<T>& ref = a.isScalar ? b : a;
  MEGBA_CHECK(!ref.isScalar, "need at least one vector operand");
  if (!a.isScalar && !b.isScalar) {
    MEGBA_CHECK(a.nItem == b.nItem, "JetVector item-count mismatch");
    MEGBA_CHECK(a.N == b.N, "JetVector gradient-width mismatch");
    MEGBA_CHECK(a.onGpu == b.onGpu, "JetVector device mismatch");
  }
  return denseLike(ref);
}

// ---------------------------------------------------------------------------
// Launcher: body(i) for every item i, on the GPU or the CPU.
// ---------------------------------------------------------------------------
template <typename Body>
__global__ void kForEach(int64_t n, Body body) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    body(i);
}

inline int jvGrid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// Body is a trivially copyable functor; it travels in the kernel arguments.
template <typename Body>
void forEachItem(bool onGpu, int64_t n, Body body) {
  if (onGpu) {
    hipLaunchKernelGGL(kForEach<Body>, dim3(jvGrid(n)), dim3(256), 0, 0, n,
                       body);
    JV_HIP_CHECK(hipGetLastError());
  } else {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) body(i);
  }
}

// f(tag) with a runtime enum value as an integral_constant tag.
template <typename F>
decltype(auto) dispatchOp(JvOp op, F&& f) {
  switch (op) {
    case JvOp::Add: return f(std::integral_constant<JvOp, JvOp::Add>{});
    case JvOp::Sub: return f(std::integral_constant<JvOp, JvOp::Sub>{});
    case JvOp::Mul: return f(std::integral_constant<JvOp, JvOp::Mul>{});
    default: return f(std::integral_constant<JvOp, JvOp::Div>{});
  }
}
template <typename F>
decltype(auto) dispatchUnary(JvUnary op, F&& f) {
  switch (op) {
    case JvUnary::Neg: return f(std::integral_constant<JvUnary, JvUnary::Neg>{});
    case JvUnary::Abs: return f(std::integral_constant<JvUnary, JvUnary::Abs>{});
    case JvUnary::Sin: return f(std::integral_constant<JvUnary, JvUnary::Sin>{});
    case JvUnary::Cos: return f(std::integral_constant<JvUnary, JvUnary::Cos>{});
    default: return f(std::integral_constant<JvUnary, JvUnary::Sqrt>{});
  }
}
template <typename F>
decltype(auto) dispatchKind(JvKind k, F&& f) {
  switch (k) {
    case JvKind::DENSE: return f(std::integral_constant<JvKind, JvKind::DENSE>{});
    case JvKind::JPV: return f(std::integral_constant<JvKind, JvKind::JPV>{});
    default: return f(std::integral_constant<JvKind, JvKind::SCALAR>{});
  }
}
// f(kindTag) for the kind of a vector operand (DENSE or JPV).
template <typename T, typename F>
void dispatchVectorKind(const JetVec<T>& a, F&& f) {
  dispatchKind(a.kind(), [&](auto k) {
    if constexpr (decltype(k)::value != JvKind::SCALAR) f(k);
  });
}

// ---------------------------------------------------------------------------
// Per-item bodies
// ---------------------------------------------------------------------------
// Operand access generic over kind, usable on host and device.
template <typename T, JvKind K>
struct Operand {
  const T* value;
  const T* grad;
  T scalar;
  int gradPos;
  int64_t n;
  MEGBA_HD inline T val(int64_t i) const {
    return K == JvKind::SCALAR ? scalar : value[i];
  }
  MEGBA_HD inline T der(int g, int64_t i) const {
    if (K == JvKind::DENSE) return grad[(int64_t)g * n + i];
    if (K == JvKind::JPV) return g == gradPos ? T(1) : T(0);
    return T(0);
  }
};

template <typename T, JvKind K>
Operand<T, K> makeOperand(const JetVec<T>& a) {
  Operand<T, K> o;
  o.value = a.value ? a.value->ptr : nullptr;
  o.grad = a.grad ? a.grad->ptr : nullptr;
  o.scalar = a.scalarVal;
  o.gradPos = a.gradPos;
  o.n = a.nItem;
  return o;
}

template <JvOp OP, typename T>
MEGBA_HD inline T binaryValue(T av, T bv) {
  if (OP == JvOp::Add) return av + bv;
  if (OP == JvOp::Sub) return av - bv;
  if (OP == JvOp::Mul) return av * bv;
  return av / bv;
}

template <typename T, JvOp OP, JvKind KA, JvKind KB>
struct BinaryItem {
  Operand<T, KA> a;
  Operand<T, KB> b;
  int64_t n;
  int N;
  T* ov;
  T* og;
  MEGBA_HD void operator()(int64_t i) const {
    const T av = a.val(i), bv = b.val(i);
    const T v = binaryValue<OP>(av, bv);
    ov[i] = v;
    for (int g = 0; g < N; ++g) {
      const T ag = a.der(g, i), bg = b.der(g, i);
      T d;
      if (OP == JvOp::Add) d = ag + bg;
      if (OP == JvOp::Sub) d = ag - bg;
      if (OP == JvOp::Mul) d = ag * bv + av * bg;
      if (OP == JvOp::Div) d = (ag - v * bg) / bv;
      og[(int64_t)g * n + i] = d;
    }
  }
};

template <typename T, JvUnary OP, JvKind K>
struct UnaryItem {
  Operand<T, K> a;
  int64_t n;
  int N;
  T* ov;
  T* og;
  MEGBA_HD void operator()(int64_t i) const {
    const T v = a.val(i);
    T outv, scale;  // d out = scale * d in
    if (OP == JvUnary::Neg) { outv = -v; scale = T(-1); }
    if (OP == JvUnary::Abs) { outv = v < T(0) ? -v : v; scale = v < T(0) ? T(-1) : T(1); }
    if (OP == JvUnary::Sin) { outv = std::sin(v); scale = std::cos(v); }
    if (OP == JvUnary::Cos) { outv = std::cos(v); scale = -std::sin(v); }
    if (OP == JvUnary::Sqrt) { outv = std::sqrt(v); scale = T(0.5) / outv; }
    ov[i] = outv;
    for (int g = 0; g < N; ++g) og[(int64_t)g * n + i] = scale * a.der(g, i);
  }
};

// wrap = theta - 2*pi*floor((theta + pi) / (2*pi)), in [-pi, pi);
// d wrap / d theta = 1.
template <typename T, JvKind K>
struct NormalizeAngleItem {
  Operand<T, K> a;
  int64_t n;
  int N;
  T* ov;
  T* og;
  MEGBA_HD void operator()(int64_t i) const {
    // No FMA: the wrapped value has the same bits on both backends.
#pragma clang fp contract(off)
    const T twoPi = T(6.283185307179586476925286766559);
    const T v = a.val(i);
    ov[i] = v - twoPi * (T)std::floor(((double)v + 3.14159265358979323846) /
                                      (double)twoPi);
    for (int g = 0; g < N; ++g) og[(int64_t)g * n + i] = a.der(g, i);
  }
};

// Rotation matrix -> unit quaternion [w,x,y,z] with gradients: per-item
// Shepperd branch b on the largest of {trace, R00, R11, R22} (the reference's
// RotationToQuaternion kernel, quaternion.cu:102-199, used a static device
// function-pointer table; here one parameterised branch).  q[b] is the major
// component sqrt(t)/2; the other three are (R[p] + sign*R[m]) / (2 sqrt(t)).
// The pointer tables travel by value (208 bytes).
template <typename T>
struct Rot2QuatItem {
  const T* rv[9];
  const T* rg[9];
  T* qv[4];
  T* qg[4];
  int64_t n;
  int N;
  MEGBA_HD void operator()(int64_t i) const {
    // No FMA: the minor components' gradients are differences that cancel
    // (to exactly 0 where q does not depend on the parameter); fused and
    // unfused products leave different residues there, so with contraction
    // the GPU gradient would not match the CPU's to any relative bound.
#pragma clang fp contract(off)
    // t = 1 + sg . (R00, R11, R22)
    const T sg[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
    // per branch, the three minor components as {component, p, m, sign}
    const int oth[4][3][4] = {
        {{1, 7, 5, -1}, {2, 2, 6, -1}, {3, 3, 1, -1}},
        {{0, 7, 5, -1}, {2, 3, 1, +1}, {3, 2, 6, +1}},
        {{0, 2, 6, -1}, {1, 3, 1, +1}, {3, 7, 5, +1}},
        {{0, 3, 1, -1}, {1, 2, 6, +1}, {2, 7, 5, +1}}};
    T v[9], q[4];
    for (int k = 0; k < 9; ++k) v[k] = rv[k][i];
    const T tr = v[0] + v[4] + v[8];
    int b = 0;
    T best = tr;
    if (v[0] > best) { b = 1; best = v[0]; }
    if (v[4] > best) { b = 2; best = v[4]; }
    if (v[8] > best) { b = 3; }
    const T t = T(1) + sg[b][0] * v[0] + sg[b][1] * v[4] + sg[b][2] * v[8];
    const T s = std::sqrt(t);
    const T inv2s = T(0.5) / s;
    q[b] = s * T(0.5);
    T comp[3];
    for (int k = 0; k < 3; ++k) {
      comp[k] = (v[oth[b][k][1]] + T(oth[b][k][3]) * v[oth[b][k][2]]) * inv2s;
      q[oth[b][k][0]] = comp[k];
    }
    for (int k = 0; k < 4; ++k) qv[k][i] = q[k];
    for (int g = 0; g < N; ++g) {
      const T dt = sg[b][0] * rg[0][(int64_t)g * n + i] +
                   sg[b][1] * rg[4][(int64_t)g * n + i] +
                   sg[b][2] * rg[8][(int64_t)g * n + i];
      const T ds = dt * inv2s;
      qg[b][(int64_t)g * n + i] = ds * T(0.5);
      for (int k = 0; k < 3; ++k) {
        const T dn = rg[oth[b][k][1]][(int64_t)g * n + i] +
                     T(oth[b][k][3]) * rg[oth[b][k][2]][(int64_t)g * n + i];
        qg[oth[b][k][0]][(int64_t)g * n + i] = dn * inv2s - comp[k] * ds / s;
      }
    }
  }
};

}  // namespace

template <typename T>
JetVec<T> jvFromHost(const T* value, const T* grad, int64_t nItem, int N,
                     int gradPos, bool onGpu) {
  JetVec<T> v;
  v.nItem = nItem;
  v.N = N;
  v.gradPos = gradPos;
  v.onGpu = onGpu;
  v.value = makeBuf<T>(nItem, onGpu);
  copyIn(onGpu, v.value->ptr, value, nItem);
  if (grad != nullptr && gradPos < 0) {
    v.grad = makeBuf<T>((int64_t)N * nItem, onGpu);
    copyIn(onGpu, v.grad->ptr, grad, (int64_t)N * nItem);
  }
  return v;
}

template <typename T>
JetVec<T> jvScalar(T s, int N) {
  JetVec<T> v;
  v.isScalar = true;
  v.scalarVal = s;
  v.N = N;
  return v;
}

template <typename T>
void jvToHost(const JetVec<T>& a, T* value, T* grad) {
  MEGBA_CHECK(!a.isScalar, "cannot download a scalar JetVector");
  copyOut(a.onGpu, value, a.value->ptr, a.nItem);
  if (!grad) return;
  if (a.grad) {
    copyOut(a.onGpu, grad, a.grad->ptr, (int64_t)a.N * a.nItem);
  } else {
    for (int g = 0; g < a.N; ++g)
      for (int64_t i = 0; i < a.nItem; ++i)
        grad[(int64_t)g * a.nItem + i] = (g == a.gradPos) ? T(1) : T(0);
  }
}

template <typename T>
JetVec<T> jvBinary(JvOp op, const JetVec<T>& a, const JetVec<T>& b) {
  if (a.isScalar && b.isScalar) {
    // Pure-scalar op: host arithmetic, scalar result (the reference's
    // PURE_SCALAR_OP dispatch, src/operator/jet_vector.cpp).
    MEGBA_CHECK(a.N == b.N, "JetVector gradient-width mismatch");
    return dispatchOp(op, [&](auto opTag) {
      return jvScalar<T>(
          binaryValue<decltype(opTag)::value>(a.scalarVal, b.scalarVal), a.N);
    });
  }
  JetVec<T> out = denseLike(a, b);
  dispatchOp(op, [&](auto opTag) {
    dispatchKind(a.kind(), [&](auto ka) {
      dispatchKind(b.kind(), [&](auto kb) {
        constexpr JvKind KA = decltype(ka)::value, KB = decltype(kb)::value;
        if constexpr (KA == JvKind::SCALAR && KB == JvKind::SCALAR) {
          MEGBA_CHECK(false, "scalar op scalar is not a JetVector op");
        } else {
          forEachItem(out.onGpu, out.nItem,
                      BinaryItem<T, decltype(opTag)::value, KA, KB>{
                          makeOperand<T, KA>(a), makeOperand<T, KB>(b),
                          out.nItem, out.N, out.value->ptr, out.grad->ptr});
        }
      });
    });
  });
  return out;
}

template <typename T>
JetVec<T> jvUnary(JvUnary op, const JetVec<T>& a) {
  MEGBA_CHECK(!a.isScalar, "unary op needs a vector operand");
  JetVec<T> out = denseLike(a);
  dispatchUnary(op, [&](auto opTag) {
    dispatchVectorKind(a, [&](auto k) {
      constexpr JvKind K = decltype(k)::value;
      forEachItem(out.onGpu, out.nItem,
                  UnaryItem<T, decltype(opTag)::value, K>{
                      makeOperand<T, K>(a), out.nItem, out.N, out.value->ptr,
                      out.grad->ptr});
    });
  });
  return out;
}

// ---------------------------------------------------------------------------
// Geometry (composed from elementwise ops; reference include/geo/geo.cuh)
// ---------------------------------------------------------------------------
namespace {
template <typename T>
JetVec<T> operator+(const JetVec<T>& a, const JetVec<T>& b) { return jvBinary(JvOp::Add, a, b); }
template <typename T>
JetVec<T> operator-(const JetVec<T>& a, const JetVec<T>& b) { return jvBinary(JvOp::Sub, a, b); }
template <typename T>
JetVec<T> operator*(const JetVec<T>& a, const JetVec<T>& b) { return jvBinary(JvOp::Mul, a, b); }
template <typename T>
JetVec<T> operator/(const JetVec<T>& a, const JetVec<T>& b) { return jvBinary(JvOp::Div, a, b); }
}  // namespace

template <typename T>
std::vector<JetVec<T>> jvAngleAxisToRotation(const std::vector<JetVec<T>>& aa) {
  MEGBA_CHECK(aa.size() == 3, "angle-axis needs 3 components");
  const int N = aa[0].N;
  auto S = [&](double v) { return jvScalar<T>((T)v, N); };
  JetVec<T> t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  // NOTE: vectorised expression form has no per-item branch; near-zero angles
  // are handled by the tiny epsilon regulariser below (matches the
  // reference's vectorised evaluation, which likewise divides by theta).
  JetVec<T> theta = jvUnary(JvUnary::Sqrt, t2 + S(1e-30));
  JetVec<T> c = jvUnary(JvUnary::Cos, theta);
  JetVec<T> s = jvUnary(JvUnary::Sin, theta);
  JetVec<T> omc = S(1.0) - c;
  std::vector<JetVec<T>> w;
  for (int i = 0; i < 3; ++i) w.push_back(aa[i] / theta);
  std::vector<JetVec<T>> R;
  R.reserve(9);
  // R = c I + s [w]x + (1-c) w w^T  (row-major)
  R.push_back(c + omc * (w[0] * w[0]));
  R.push_back(omc * (w[0] * w[1]) - s * w[2]);
  R.push_back(omc * (w[0] * w[2]) + s * w[1]);
  R.push_back(omc * (w[1] * w[0]) + s * w[2]);
  R.push_back(c + omc * (w[1] * w[1]));
  R.push_back(omc * (w[1] * w[2]) - s * w[0]);
  R.push_back(omc * (w[2] * w[0]) - s * w[1]);
  R.push_back(omc * (w[2] * w[1]) + s * w[0]);
  R.push_back(c + omc * (w[2] * w[2]));
  return R;
}

// The wrap has a per-item branch (floor), so it is a body of its own and not
// a composition of elementwise ops.
template <typename T>
JetVec<T> jvNormalizeAngle(const JetVec<T>& theta) {
  MEGBA_CHECK(!theta.isScalar, "normalize_angle needs a vector operand");
  JetVec<T> out = denseLike(theta);
  dispatchVectorKind(theta, [&](auto k) {
    constexpr JvKind K = decltype(k)::value;
    forEachItem(out.onGpu, out.nItem,
                NormalizeAngleItem<T, K>{makeOperand<T, K>(theta), out.nItem,
                                         out.N, out.value->ptr,
                                         out.grad->ptr});
  });
  return out;
}
template JetVec<double> jvNormalizeAngle<double>(const JetVec<double>&);
template JetVec<float> jvNormalizeAngle<float>(const JetVec<float>&);

template <typename T>
std::vector<JetVec<T>> jvRotation2D(const JetVec<T>& theta) {
  JetVec<T> c = jvUnary(JvUnary::Cos, theta);
  JetVec<T> s = jvUnary(JvUnary::Sin, theta);
  return {c, jvUnary(JvUnary::Neg, s), s, c};
}

template <typename T>
std::vector<JetVec<T>> jvQuaternionToRotation(const std::vector<JetVec<T>>& q) {
  MEGBA_CHECK(q.size() == 4, "quaternion needs 4 components");
  const int N = q[0].N;
  auto S = [&](double v) { return jvScalar<T>((T)v, N); };
  const JetVec<T>&w = q[0], &x = q[1], &y = q[2], &z = q[3];
  JetVec<T> two = S(2.0);
  std::vector<JetVec<T>> R;
  R.push_back(S(1.0) - two * (y * y + z * z));
  R.push_back(two * (x * y - w * z));
  R.push_back(two * (x * z + w * y));
  R.push_back(two * (x * y + w * z));
  R.push_back(S(1.0) - two * (x * x + z * z));
  R.push_back(two * (y * z - w * x));
  R.push_back(two * (x * z - w * y));
  R.push_back(two * (y * z + w * x));
  R.push_back(S(1.0) - two * (x * x + y * y));
  return R;
}

template <typename T>
std::vector<JetVec<T>> jvNormalizeQuaternion(const std::vector<JetVec<T>>& q) {
  MEGBA_CHECK(q.size() == 4, "quaternion needs 4 components");
  JetVec<T> n = jvUnary(
      JvUnary::Sqrt, q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  std::vector<JetVec<T>> out;
  for (int i = 0; i < 4; ++i) out.push_back(q[i] / n);
  return out;
}

template <typename T>
JetVec<T> jvRadialDistortion(const std::vector<JetVec<T>>& p,
                             const std::vector<JetVec<T>>& intr) {
  MEGBA_CHECK(p.size() >= 2 && intr.size() == 3,
              "radial distortion needs p[>=2], intr[3]");
  const int N = intr[0].N;
  JetVec<T> r2 = p[0] * p[0] + p[1] * p[1];
  JetVec<T> d = jvScalar<T>(T(1), N) + r2 * (intr[1] + intr[2] * r2);
  return intr[0] * d;
}

// Inputs must be dense JetVectors (geometry-op outputs are).
template <typename T>
std::vector<JetVec<T>> jvRotationToQuaternion(const std::vector<JetVec<T>>& R) {
  MEGBA_CHECK(R.size() == 9, "rotation needs 9 components");
  for (const auto& r : R)
    MEGBA_CHECK(r.kind() == JvKind::DENSE, "rot->quat needs dense JetVectors");
  std::vector<JetVec<T>> q;
  Rot2QuatItem<T> body;
  body.n = R[0].nItem;
  body.N = R[0].N;
  for (int k = 0; k < 9; ++k) {
    body.rv[k] = R[k].value->ptr;
    body.rg[k] = R[k].grad->ptr;
  }
  for (int k = 0; k < 4; ++k) {
    q.push_back(denseLike(R[0]));
    body.qv[k] = q[k].value->ptr;
    body.qg[k] = q[k].grad->ptr;
  }
  forEachItem(R[0].onGpu, body.n, body);
  return q;
}
template std::vector<JetVec<double>> jvRotationToQuaternion<double>(
    const std::vector<JetVec<double>>&);
template std::vector<JetVec<float>> jvRotationToQuaternion<float>(
    const std::vector<JetVec<float>>&);

// Explicit instantiations.
#define JV_INST(T)                                                            \
  template JetVec<T> jvFromHost<T>(const T*, const T*, int64_t, int, int,     \
                                   bool);                                     \
  template JetVec<T> jvScalar<T>(T, int);                                     \
  template void jvToHost<T>(const JetVec<T>&, T*, T*);                        \
  template JetVec<T> jvBinary<T>(JvOp, const JetVec<T>&, const JetVec<T>&);   \
  template JetVec<T> jvUnary<T>(JvUnary, const JetVec<T>&);                   \
  template std::vector<JetVec<T>> jvAngleAxisToRotation<T>(                   \
      const std::vector<JetVec<T>>&);                                         \
  template std::vector<JetVec<T>> jvRotation2D<T>(const JetVec<T>&);          \
  template std::vector<JetVec<T>> jvQuaternionToRotation<T>(                  \
      const std::vector<JetVec<T>>&);                                         \
  template std::vector<JetVec<T>> jvNormalizeQuaternion<T>(                   \
      const std::vector<JetVec<T>>&);                                         \
  template JetVec<T> jvRadialDistortion<T>(const std::vector<JetVec<T>>&,     \
                                           const std::vector<JetVec<T>>&);
JV_INST(double)
JV_INST(float)
#undef JV_INST

}  // namespace megba
