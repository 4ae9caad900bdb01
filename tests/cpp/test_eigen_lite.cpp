// The Eigen stand-in (third_party/eigen_lite) on the host: the members the tree
// calls, storage order, the comma initialiser, conversions between static
// shapes, Map views, the triangular solves, and the element lifetimes of a
// scalar that needs initialisation.  Prints "ok"; no device call.
#include <Eigen/Dense>
#include <cstdio>
#include <vector>
#include <cmath>
static int live = 0;
struct Tr { double v; Tr() : v(0) { ++live; } Tr(double x) : v(x) { ++live; } Tr(const Tr& o) : v(o.v) { ++live; } ~Tr() { --live; }
  Tr& operator=(const Tr&) = default; Tr& operator+=(const Tr& o){v+=o.v;return *this;} };
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
int main() {
  using namespace Eigen;
  {
    MatrixXd A(3, 3); A << 2, 0, 0, 1, 3, 0, 4, 5, 6;
    CHECK(A(1, 0) == 1 && A(2, 1) == 5 && A.data()[1] == 1);
    VectorXd b(3); b << 2, 7, 32;
    VectorXd x = A.triangularView<Lower>().solve(b);
    CHECK(std::fabs(x(0) - 1) < 1e-15 && std::fabs(x(1) - 2) < 1e-15 && std::fabs(x(2) - 3) < 1e-15);
    MatrixXd At = A.transpose();
    VectorXd bu(3); bu << 2*1+1*2+4*3, 3*2+5*3, 18;
    VectorXd xu = At.triangularView<Upper>().solve(bu);
    CHECK(std::fabs(xu(0) - 1) < 1e-14 && std::fabs(xu(2) - 3) < 1e-14);
    MatrixXd I = MatrixXd::Identity(3, 3);
    MatrixXd Ai = A.triangularView<Lower>().solve(I);
    CHECK(std::fabs(Ai(0,0) - 0.5) < 1e-15 && Ai(0, 2) == 0);
    RowVectorXd r = b.transpose(); CHECK(r.rows() == 1 && r.cols() == 3 && r(2) == 32);
    MatrixXd M(r); CHECK(M.rows() == 1 && M.cols() == 3);
    MatrixXd M2 = b; CHECK(M2.rows() == 3 && M2.cols() == 1);
    VectorXd t = b.tail(2); CHECK(t.size() == 2 && t(0) == 7);
    VectorXd h = b.head(2).eval(); CHECK(h(1) == 7);
    CHECK(b.sum() == 41); VectorXd s = b * 0.5; CHECK(s(0) == 1);
    std::vector<double> raw{1, 2, 3, 4, 5, 6};
    MatrixXd Q = Map<const MatrixXd>(raw.data(), 2, 3); CHECK(Q(1, 2) == 6 && Q(0, 1) == 3);
    Map<VectorXd> v(raw.data(), 6); v.setZero(); CHECK(raw[5] == 0);
    v(2) = 9; CHECK(raw[2] == 9);
    VectorXd g; g = Map<VectorXd>(raw.data(), 6); CHECK(g.size() == 6 && g(2) == 9);
    MatrixXd out(4, 0); out.resize(NoChange, 5); CHECK(out.rows() == 4 && out.cols() == 5);
    std::vector<VectorXd> vs(3, VectorXd::Zero(2)); vs[1] = VectorXd::Ones(4); CHECK(vs[1].size() == 4 && vs[0](1) == 0);
    Matrix<double, -1, 1> e0(0); CHECK(e0.size() == 0);
    MatrixXd mv = std::move(Q); CHECK(Q.size() == 0 && mv(1, 2) == 6);
    Q = mv; mv = MatrixXd(); CHECK(Q(1, 2) == 6 && mv.size() == 0);
    Matrix<int, -1, -1> ci = Q.cast<int>(); CHECK(ci(1, 2) == 6);
  }
  {
    Matrix<Tr, -1, -1> A(2, 2); CHECK(live == 4);
    Matrix<Tr, -1, -1> B = A; CHECK(live == 8);
    B.resize(3, 3); CHECK(live == 13);
    A = B; CHECK(live == 18);
    Matrix<Tr, -1, 1> v(3); v << 1, 2, 3; CHECK(v(2).v == 3);
    Matrix<Tr, -1, -1> C = v; CHECK(C.rows() == 3);
    Matrix<Tr, -1, 1> z = Matrix<Tr, -1, 1>::Zero(5); CHECK(z.size() == 5);
    Matrix<Tr, -1, 1> w = std::move(z); CHECK(z.size() == 0);
    w = Matrix<Tr, -1, 1>(2);
  }
  CHECK(live == 0);
  std::printf("ok\n");
  return 0;
}
