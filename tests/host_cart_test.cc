// Stand-alone host program for the host side of the decision-tree section of include/amx.h: it compiles rasr_amd/csrc/cart.hip's host side
// into itself (no librasr_amd.so, no Python), walks through every refusal of amx_cart_train and its message, and runs whole trainings of
// the host's tree -- node lists, question-id lists, the priority queue's heap moves, the look-ahead, rollback, numbering -- with the two
// device seams of amx::CartTraining (upload_device, compute) replaced by plain loops that do what cart_eval_kernel does, in its order.
// No device call is made.  Each training is held to what must be true of any result (a split's gain is father - (left + right) in every
// bit, the counts add up, orders and classes are permutations, the log's running total is its own chain), and the default mode to
// exact_all.  Meant to be built with the host sanitizers (tests/test_cart.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_cart_test.cc -o host_cart_test && ./host_cart_test
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/cart.hip"

// what api.cpp gives the library
static std::string g_error;
namespace amx {
void set_error(const char* fmt, ...) {
    char    buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace amx

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("%s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

static bool says(const char* what) { return g_error.find(what) != std::string::npos; }

// the device seams as plain loops: what cart_eval_kernel computes for every (node, question), in list order
struct HostTraining : amx::CartTraining {
    HostTraining(const amx_cart_problem& p, const amx_cart_plan& pl, bool fused) : amx::CartTraining(nullptr, p, pl, fused) {}
    int upload_device() override { return AMX_OK; }
    int compute(const std::vector<amx::CartTask>& tasks, const std::vector<int>& list, const std::vector<int>& qrows, long long items, amx::CartCount* cnt,
                double* screen, double* sums) override {
        std::vector<double> l((size_t)R), r((size_t)R);
        for (const amx::CartTask& t : tasks)
            for (int q = 0; q < t.n_q; ++q) {
                const uint32_t* bits = pb.answers + (size_t)qrows[(size_t)(t.q0 + q)] * words;
                amx::CartCount  k{0, 0, 0, 0};
                std::fill(l.begin(), l.end(), 0.0), std::fill(r.begin(), r.end(), 0.0);
                for (int e = 0; e < t.n_ex; ++e) {
                    const int  idx = list[(size_t)(t.list0 + e)];
                    const bool bit = (bits[idx >> 5] >> (idx & 31)) & 1u;
                    for (int c = 0; c < R; ++c) {
                        const double v = rows[(size_t)idx * R + c];
                        l[(size_t)c] += bit ? v : 0.0;
                        r[(size_t)c] += bit ? 0.0 : v;
                    }
                    const double w = rows[(size_t)idx * R];
                    if (bit)
                        k.l_obs = (unsigned)((double)k.l_obs + w), ++k.l_ex;
                    else
                        k.r_obs = (unsigned)((double)k.r_obs + w), ++k.r_ex;
                }
                const long long item = t.out0 + q;
                if (item < 0 || item >= items)
                    return AMX_ERR_STATE;
                cnt[item] = k;
                if (sums) {
                    std::memcpy(sums + (size_t)item * 2 * R, l.data(), (size_t)R * sizeof(double));
                    std::memcpy(sums + (size_t)item * 2 * R + R, r.data(), (size_t)R * sizeof(double));
                }
                if (screen) {
                    double       al, ar;
                    const double a = fma ? amx::cart_likelihood<true>(l.data(), k.l_ex, pb.dim, plan.variance_clipping, &al)
                                         : amx::cart_likelihood<false>(l.data(), k.l_ex, pb.dim, plan.variance_clipping, &al);
                    const double b = fma ? amx::cart_likelihood<true>(r.data(), k.r_ex, pb.dim, plan.variance_clipping, &ar)
                                         : amx::cart_likelihood<false>(r.data(), k.r_ex, pb.dim, plan.variance_clipping, &ar);
                    screen[2 * item]     = t.father - (a + b);
                    screen[2 * item + 1] = 2.0 * (amx::cart_side_margin(l[0], pb.dim, al, a) + amx::cart_side_margin(r[0], pb.dim, ar, b)) +
                                           8.0 * amx::kCartEps * (fabs(a) + fabs(b) + fabs(t.father));
                }
            }
        return AMX_OK;
    }
};

struct Problem {
    int                   E, dim, Q;
    std::vector<double>   n_obs, values;
    std::vector<uint32_t> answers;
    amx_cart_problem view() const { return amx_cart_problem{E, dim, Q, n_obs.data(), values.data(), answers.data()}; }
    bool answer(int q, int e) const { return (answers[(size_t)q * ((E + 31) / 32) + (e >> 5)] >> (e & 31)) & 1u; }
};

static unsigned long long g_rng = 88172645463325252ull;
static double uniform() {   // xorshift64
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}

// E examples as sums over a few frames around a centre of their own; fractional: weights that are no whole numbers; twins: the second
// half mirrors the first and question 0 tells the halves apart (equal gains wait in the queue)
static Problem make(int E, int dim, int Q, bool fractional, bool twins) {
    Problem p;
    p.E = E, p.dim = dim, p.Q = Q;
    p.n_obs.assign((size_t)E, 0.0), p.values.assign((size_t)E * 2 * dim, 0.0);
    const int words = (E + 31) / 32;
    p.answers.assign((size_t)Q * words, 0u);
    for (int e = 0; e < E; ++e) {
        const int n = 1 + (int)(uniform() * 12);
        std::vector<double> centre((size_t)dim);
        for (double& c : centre)
            c = 4.0 * uniform() - 2.0 + (twins ? 3.0 : 0.0);
        for (int i = 0; i < n; ++i) {
            const double w = fractional ? 0.05 + 1.4 * uniform() : 1.0;
            p.n_obs[(size_t)e] += w;
            for (int d = 0; d < dim; ++d) {
                const double x = centre[(size_t)d] + uniform() - 0.5;
                p.values[(size_t)e * 2 * dim + d] += x * w;
                p.values[(size_t)e * 2 * dim + dim + d] += x * x * w;
            }
        }
    }
    for (int q = 0; q < Q; ++q) {
        const double share = 0.2 + 0.6 * uniform();
        for (int e = 0; e < E; ++e)
            if (uniform() < share)
                p.answers[(size_t)q * words + (e >> 5)] |= 1u << (e & 31);
    }
    if (twins) {
        const int half = E / 2;
        for (int e = 0; e < half; ++e) {
            p.n_obs[(size_t)(half + e)] = p.n_obs[(size_t)e];
            for (int d = 0; d < dim; ++d) {
                p.values[(size_t)(half + e) * 2 * dim + d]       = -p.values[(size_t)e * 2 * dim + d];
                p.values[(size_t)(half + e) * 2 * dim + dim + d] = p.values[(size_t)e * 2 * dim + dim + d];
            }
            for (int q = 0; q < Q; ++q) {
                const bool a = q == 0 ? false : p.answer(q, e);
                uint32_t&  w = p.answers[(size_t)q * words + ((half + e) >> 5)];
                w            = a ? w | (1u << ((half + e) & 31)) : w & ~(1u << ((half + e) & 31));
                if (q == 0)
                    p.answers[(size_t)(e >> 5)] |= 1u << (e & 31);
            }
        }
    }
    return p;
}

static bool run(const Problem& p, const amx_cart_plan& plan, bool fused, amx_cart_tree* tree) {
    const amx_cart_problem v = p.view();
    CHECK(amx::cart_check(&v, &plan, "host_cart_test") == AMX_OK);
    HostTraining t(v, plan, fused);
    const int    st = t.train(tree);
    CHECK(st == AMX_OK);
    return st == AMX_OK;
}

static bool same(const amx_cart_tree& a, const amx_cart_tree& b) {
    if (a.nodes.size() != b.nodes.size() || a.log.size() != b.log.size() || a.classes != b.classes || a.qstats.size() != b.qstats.size())
        return false;
    for (size_t i = 0; i < a.nodes.size(); ++i)
        if (std::memcmp(&a.nodes[i].score, &b.nodes[i].score, 8) || a.nodes[i].left != b.nodes[i].left || a.nodes[i].right != b.nodes[i].right ||
            a.nodes[i].step != b.nodes[i].step || a.nodes[i].row != b.nodes[i].row || a.nodes[i].n_obs != b.nodes[i].n_obs ||
            a.nodes[i].class_id != b.nodes[i].class_id || a.nodes[i].depth != b.nodes[i].depth)
            return false;
    for (size_t i = 0; i < a.log.size(); ++i)
        if (a.log[i].node != b.log[i].node || a.log[i].row != b.log[i].row || std::memcmp(&a.log[i].gain, &b.log[i].gain, 8) ||
            std::memcmp(&a.log[i].total_gain, &b.log[i].total_gain, 8))
            return false;
    for (size_t i = 0; i < a.qstats.size(); ++i)
        if (a.qstats[i].count != b.qstats[i].count || std::memcmp(&a.qstats[i].sum_gain, &b.qstats[i].sum_gain, 8))
            return false;
    return a.info.negative_gain_errors == b.info.negative_gain_errors && a.info.n_leaves == b.info.n_leaves && a.info.n_obs == b.info.n_obs;
}

// what must be true of any result
static void consistent(const Problem& p, const amx_cart_plan& plan, const amx_cart_tree& t) {
    const int n = (int)t.nodes.size();
    CHECK(n == t.info.n_nodes && n == 2 * (int)t.log.size() + 1 && t.info.n_leaves == (int)t.log.size() + 1);
    CHECK((unsigned)t.info.n_leaves <= plan.max_leaves || t.log.empty());
    std::vector<int> parent((size_t)n, -1), leaf_seen((size_t)t.info.n_leaves, 0);
    double           total = 0.0;
    int              next  = 1;
    for (const amx_cart_commit& c : t.log) {
        CHECK(c.node >= 0 && c.node < n);
        const amx_cart_node& f = t.nodes[(size_t)c.node];
        CHECK(f.left == next && f.right == next + 1 && f.step == c.step && f.row == c.row && f.depth == c.depth);   // insertSplit numbers in commit order
        next += 2;
        const amx_cart_node &l = t.nodes[(size_t)f.left], &r = t.nodes[(size_t)f.right];
        const double         gain = f.score - (l.score + r.score);
        CHECK(std::memcmp(&gain, &c.gain, 8) == 0);
        CHECK(c.gain > 0.0 && c.gain >= plan.steps[c.step].min_gain);
        CHECK(l.n_obs >= plan.steps[c.step].min_obs && r.n_obs >= plan.steps[c.step].min_obs && l.n_obs > 0 && r.n_obs > 0);
        CHECK(l.depth == f.depth + 1 && r.depth == f.depth + 1);
        total += c.gain;
        CHECK(std::memcmp(&total, &c.total_gain, 8) == 0);
        parent[(size_t)f.left] = parent[(size_t)f.right] = c.node;
    }
    CHECK(std::memcmp(&total, &t.info.total_gain, 8) == 0);
    for (int i = 0; i < n; ++i) {
        const amx_cart_node& x = t.nodes[(size_t)i];
        CHECK((i == 0) == (parent[(size_t)i] < 0));
        if (x.left < 0) {
            CHECK(x.right < 0 && x.step < 0 && x.row < 0 && x.class_id >= 0 && x.class_id < t.info.n_leaves);
            if (x.class_id >= 0 && x.class_id < t.info.n_leaves)
                ++leaf_seen[(size_t)x.class_id];
        }
        else
            CHECK(x.class_id == -1);
    }
    for (int s : leaf_seen)
        CHECK(s == 1);
    // every example sits in the leaf its answers lead to
    for (int e = 0; e < p.E; ++e) {
        int i = 0;
        while (t.nodes[(size_t)i].left >= 0)
            i = p.answer(t.nodes[(size_t)i].row, e) ? t.nodes[(size_t)i].left : t.nodes[(size_t)i].right;
        CHECK(t.classes[(size_t)e] == t.nodes[(size_t)i].class_id);
    }
    unsigned long long commits = 0;
    for (const amx_cart_qstat& q : t.qstats)
        commits += q.count;
    CHECK(commits == t.log.size());
}

static void refusals() {
    Problem              p = make(8, 2, 3, false, false);
    amx_cart_problem     v = p.view();
    const int            rows[3] = {0, 1, 2};
    amx_cart_step        s{AMX_CART_SPLIT, 0, 0.0, 1, 3, rows};
    amx_cart_plan        plan{UINT_MAX, 1, &s, 0.0, 0};
    amx_cart_tree*       tree = (amx_cart_tree*)1;
    CHECK(amx_cart_train(nullptr, &v, &plan, &tree) == AMX_ERR_STATE && tree == nullptr && says("no context"));
    CHECK(amx_cart_train(nullptr, &v, &plan, nullptr) == AMX_ERR_INVALID);
    CHECK(amx_cart_train(nullptr, nullptr, &plan, &tree) == AMX_ERR_INVALID && says("NULL problem or plan"));
    amx_cart_problem b = v;
    b.n_examples       = 0;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_INVALID && says("n_examples 0"));
    b = v, b.dim = 0;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_INVALID && says("dim 0"));
    b = v, b.dim = 1025;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_UNSUPPORTED && says("dim 1025"));
    b = v, b.values = nullptr;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_INVALID && says("NULL n_obs or values"));
    b = v, b.answers = nullptr;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_INVALID && says("NULL answers"));
    Problem neg = p;
    neg.n_obs[5] = -1.0;
    b            = neg.view();
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_INVALID && says("n_obs[5] = -1"));
    neg.n_obs[5] = 4294967296.0;
    CHECK(amx_cart_train(nullptr, &b, &plan, &tree) == AMX_ERR_UNSUPPORTED && says("32 bits"));
    amx_cart_step t = s;
    amx_cart_plan q = plan;
    q.steps         = &t;
    t.randomize     = 2;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_UNSUPPORTED && says("step 0: randomize 2"));
    t = s, t.randomize = 0;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_INVALID && says("randomize 0"));
    t = s, t.action = 3;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_INVALID && says("unknown action 3"));
    const int bad_rows[3] = {0, 3, 1};
    t = s, t.questions = bad_rows;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_INVALID && says("questions[1] = 3 of 3 rows"));
    t = s, t.questions = nullptr;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_INVALID && says("NULL questions"));
    q = plan, q.variance_clipping = NAN;
    CHECK(amx_cart_train(nullptr, &v, &q, &tree) == AMX_ERR_INVALID && says("variance_clipping"));
    CHECK(amx_cart_accumulate_dev(nullptr, nullptr, 4, 4, 1, nullptr, nullptr, 3, nullptr) == AMX_ERR_INVALID && says("NULL context"));
    CHECK(amx_cart_accumulator_size(10, 40) == 810 && amx_cart_accumulator_size(-1, 40) == 0 && amx_cart_accumulator_size(3, 0) == 0);
    int stage = 0, tile = 0;
    amx_cart_kernel_shape(40, &stage, &tile);
    CHECK(stage == 50 && tile == 3);
    amx_cart_kernel_shape(1, &stage, &tile);
    CHECK(stage == 64 && tile == 85);
    amx_cart_kernel_shape(1024, &stage, &tile);
    CHECK(stage == 1 && tile == 1);
    amx_cart_kernel_shape(1025, &stage, &tile);
    CHECK(stage == 0 && tile == 0);
}

static void small_pieces() {
    CHECK(amx::cart_almost_zero(-1e-46) && amx::cart_almost_zero(-20 * 1.401298464324817e-45) && !amx::cart_almost_zero(-21 * 1.401298464324817e-45));
    CHECK(!amx::cart_almost_zero(-1e-30) && !amx::cart_almost_zero(-1.0));
    // the heap against the rule it follows: the top is never preceded by anyone; equal gains leave in an order that is the heap's own
    amx::CartQueue              q;
    std::vector<amx::CartSplit> s(40);
    for (size_t i = 0; i < s.size(); ++i) {
        s[i].gain = (double)((i * 7) % 5);
        q.insert(&s[i]);
    }
    double last = 1e300;
    size_t left = s.size();
    while (!q.empty()) {
        CHECK(q.top()->gain <= last && q.size() == left);
        last = q.top()->gain;
        q.pop();
        --left;
    }
    const double one[3] = {2.0, 6.0, 26.0};   // n = 2, mean 3, variance 13 - 9 = 4
    const double ll     = amx::cart_likelihood<false>(one, 1, 1, 0.0, nullptr);
    CHECK(ll == (0.5 * 2.0) * ((1.0 + 1.0 * amx::kCartLog2Pi) + log(4.0)));
    CHECK(amx::cart_likelihood<false>(one, 0, 1, 0.0, nullptr) == 0.0);
    CHECK(amx::cart_likelihood<false>(one, 1, 1, 5.0, nullptr) == (0.5 * 2.0) * ((1.0 + 1.0 * amx::kCartLog2Pi) + log(5.0)));
    CHECK(amx::kCartLog2Pi == log(3.141592653589793238462643383279502884197169399375105820975E+0000 + 3.141592653589793238462643383279502884197169399375105820975E+0000));
}

static void trainings() {
    struct Case {
        int      E, dim, Q;
        bool     fractional, twins;
        int      actions[3];
        unsigned min_obs, max_leaves;
        double   min_gain, clip;
    };
    const Case cases[] = {
        {1, 2, 3, false, false, {AMX_CART_SPLIT, -1, -1}, 0, UINT_MAX, 0.0, 0.0},
        {40, 3, 9, false, false, {AMX_CART_SPLIT, -1, -1}, 6, UINT_MAX, 0.0, 0.0},
        {90, 5, 12, true, false, {AMX_CART_SPLIT, -1, -1}, 5, 11, 0.0, 0.0},
        {70, 4, 12, true, false, {AMX_CART_PARTITION, AMX_CART_CLUSTER, AMX_CART_SPLIT}, 8, 30, 0.5, 0.0},
        {64, 4, 10, false, true, {AMX_CART_SPLIT, -1, -1}, 4, 21, 0.0, 0.0},
        {30, 2, 6, true, false, {AMX_CART_SPLIT, -1, -1}, 0, UINT_MAX, 0.0, 1e-2},
        {120, 40, 7, false, false, {AMX_CART_SPLIT, AMX_CART_SPLIT, -1}, 20, 9, 0.0, 0.0},
    };
    for (const Case& c : cases) {
        Problem                    p = make(c.E, c.dim, c.Q, c.fractional, c.twins);
        std::vector<int>           rows((size_t)c.Q);
        std::vector<amx_cart_step> steps;
        for (int q = 0; q < c.Q; ++q)
            rows[(size_t)q] = q;
        int n_steps = 0;
        while (n_steps < 3 && c.actions[n_steps] >= 0)
            ++n_steps;
        for (int s = 0; s < n_steps; ++s) {   // the steps share out the questions; the last one takes them all
            const int first = s + 1 == n_steps ? 0 : s * (c.Q / n_steps), count = s + 1 == n_steps ? c.Q : c.Q / n_steps;
            steps.push_back(amx_cart_step{c.actions[s], c.min_obs, c.min_gain, 1, count, rows.data() + first});
        }
        for (int fused = 0; fused < 2; ++fused) {
            amx_cart_plan plan{c.max_leaves, n_steps, steps.data(), c.clip, 1};
            amx_cart_tree exact, screened;
            if (!run(p, plan, fused != 0, &exact))
                continue;
            consistent(p, plan, exact);
            CHECK(exact.info.items_screened == 0 && exact.info.items_reevaluated > 0);
            plan.exact_all = 0;
            if (!run(p, plan, fused != 0, &screened))
                continue;
            CHECK(same(exact, screened));
            CHECK(screened.info.items_reevaluated <= screened.info.items_screened);
            if (c.E == 1)
                CHECK(exact.nodes.size() == 1 && exact.nodes[0].class_id == 0 && exact.classes[0] == 0);
            if (c.max_leaves != UINT_MAX)
                CHECK((unsigned)exact.info.n_leaves <= c.max_leaves);
            if (c.E == 40) {
                CHECK(exact.log.size() >= 1);
                // one commit at least: the root's right child is numbered before its left one's subtree
                const amx_cart_node& root = exact.nodes[0];
                int                  i    = root.right;
                while (exact.nodes[(size_t)i].left >= 0)
                    i = exact.nodes[(size_t)i].right;
                CHECK(exact.nodes[(size_t)i].class_id == 0);
            }
        }
    }
}

int main() {
    refusals();
    small_pieces();
    trainings();
    if (g_failed) {
        std::printf("host_cart_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("host_cart_test: ok\n");
    return 0;
}
