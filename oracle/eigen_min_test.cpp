// eigen_min_test.cpp -- extern "C" entry points onto the operations of oracle/eigen_min, for their unit tests
// (tests/test_kroeger_pin.py::test_eigen_min_*).  TEST INFRASTRUCTURE ONLY; built from this project's sources alone
// (`make -C oracle libeigen_min_test.so`), so the tests run wherever the oracle builds.
#include <Eigen/Core>
#include <Eigen/LU>
#include <Eigen/Dense>

extern "C" {

// out[0] = v.sum(), out[1] = (v.array() * w.array()).sum(), out[2] = v.lpNorm<1>()  (dynamic column vectors of length n)
void kroeger_eigen_redux(const float *v, const float *w, int n, float *out)
{
  Eigen::Matrix<float, Eigen::Dynamic, 1> a, b;
  a.resize(n, 1);
  b.resize(n, 1);
  for (int i = 0; i < n; ++i) { a[i] = v[i]; b[i] = w[i]; }
  out[0] = a.sum();
  out[1] = (a.array() * b.array()).sum();
  out[2] = a.lpNorm<1>();
}

// out[0] = u.squaredNorm(), out[1] = u.norm() (Vector2f); out[2] = H.determinant() (2x2, row-major h)
void kroeger_eigen_fixed(const float *u, const float *h, float *out)
{
  Eigen::Vector2f a;
  a[0] = u[0]; a[1] = u[1];
  Eigen::Matrix<float, 2, 2> H;
  H(0, 0) = h[0]; H(0, 1) = h[1]; H(1, 0) = h[2]; H(1, 1) = h[3];
  out[0] = a.squaredNorm();
  out[1] = a.norm();
  out[2] = H.determinant();
}

// H.llt() for n = 1 or 2 (row-major h): lower triangle of the factor in l (row-major, upper entries as copied), the solve of
// b in x; returns the index where the factorisation stopped, or -1
int kroeger_eigen_llt(int n, const float *h, const float *b, float *l, float *x)
{
  if (n == 1) {
    Eigen::Matrix<float, 1, 1> H, B;
    H(0, 0) = h[0]; B[0] = b[0];
    Eigen::LLT<Eigen::Matrix<float, 1, 1> > f = H.llt();
    Eigen::Matrix<float, 1, 1> X = f.solve(B);
    l[0] = f.matrixLLT()(0, 0); x[0] = X[0];
    return f.failedAt();
  }
  Eigen::Matrix<float, 2, 2> H;
  H(0, 0) = h[0]; H(0, 1) = h[1]; H(1, 0) = h[2]; H(1, 1) = h[3];
  Eigen::Vector2f B;
  B[0] = b[0]; B[1] = b[1];
  Eigen::LLT<Eigen::Matrix<float, 2, 2> > f = H.llt();
  Eigen::Vector2f X = f.solve(B);
  for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) l[r * 2 + c] = f.matrixLLT()(r, c);
  x[0] = X[0]; x[1] = X[1];
  return f.failedAt();
}

}  // extern "C"
