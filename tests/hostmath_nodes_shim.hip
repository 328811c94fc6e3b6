// TEST-ONLY host shim of the node pose transform's per-point math (csrc/nodes_math.h, the functions the kernels of csrc/nodes.hip
// run) on the CPU, so that tests/test_node_pose_cpu.py can compare it with float64 autograd without a GPU.  Not part of libbds.so,
// never loaded by the product.  Every point carries its own instance row (q [n,4], t [n,3], fv [n]).
#include "../bilateral_driving_amd/csrc/nodes_math.h"

using namespace bds;

extern "C" void hm_node_fwd(int n, const float *q, const float *t, const float *m, const float *qp, const float *logit, const float *fv,
                            float *wm, float *wq, float *op) {
  for (int i = 0; i < n; i++)
    np_forward(q + i * 4, t + i * 3, q + i * 4, m + i * 3, qp + i * 4, logit[i], fv[i], wm + i * 3, wq + i * 4, op + i);
}

// the point gradients and, per point, the instance chain of its own part (v_q [n,4], v_t [n,3])
extern "C" void hm_node_bwd(int n, const float *q, const float *m, const float *qp, const float *logit, const float *fv, const float *v_wm,
                            const float *v_wq, const float *v_op, float *v_m, float *v_qp, float *v_logit, float *v_q, float *v_t) {
  for (int i = 0; i < n; i++) {
    float part[kNpSlab];
    np_backward(q + i * 4, m + i * 3, qp + i * 4, logit[i], fv[i], v_wm + i * 3, v_wq + i * 4, v_op[i], v_m + i * 3, v_qp + i * 4,
                v_logit + i, part);
    np_instance_chain(q + i * 4, part, v_q + i * 4, v_t + i * 3);
  }
}

extern "C" void hm_node_interp(int n, const float *q1, const float *q2, float *o) {
  for (int i = 0; i < n; i++) np_interp_quats(q1 + i * 4, q2 + i * 4, o + i * 4);
}
