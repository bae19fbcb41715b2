// Test-only driver of the drop-in C++ classes (api/ over libasr_amd.so): a
// stand-alone program, as a user of those classes would write one, so that
// the GPU tests of tests/test_dropin.py need nothing outside the repository.
//
//   api_driver linear M K N        < input[M*K] weight[K*N] bias[N]
//   api_driver rnn T B In H        < input[T*B*In] w_ih[In*H] w_hh[H*H] b_ih[H] b_hh[H]
//   api_driver ctc VOCAB T B BEAM BLANK   < probabilities[T*B*V]
//
// Numbers are read from stdin, whitespace separated.  linear / rnn print the
// output matrix, one row per line; ctc first runs a randomly initialised
// Linear x3 -> RNN -> Linear x2 model through the classes (as an application
// would before decoding), then prints one "best <string> <probability>" line
// per utterance.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "CTCBeamSearch.h"
#include "Linear.h"
#include "RNN.h"
#include "cuMatrix.h"

static std::vector<float> read_floats(size_t n) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; i++)
        if (scanf("%f", &v[i]) != 1) {
            fprintf(stderr, "api_driver: expected %zu more numbers on stdin\n", n - i);
            exit(2);
        }
    return v;
}

static void print_rows(cuMatrix<float>* m) {
    m->toCpu();
    for (int i = 0; i < m->getRows(); i++) {
        for (int j = 0; j < m->getCols(); j++) printf("%s%.7f", j ? " " : "", m->get(i, j, 0));
        printf("\n");
    }
}

static int run_linear(int M, int K, int N) {
    std::vector<float> x = read_floats((size_t)M * K), w = read_floats((size_t)K * N), b = read_floats(N);
    cuMatrix<float> in(x.data(), M, K, 1);
    in.toGpu();
    Linear layer(M, K, N);
    layer.initParams(w.data(), b.data());
    print_rows(layer.forward(&in));
    return 0;
}

static int run_rnn(int T, int B, int In, int H) {
    std::vector<float> x = read_floats((size_t)T * B * In), w_ih = read_floats((size_t)In * H),
                       w_hh = read_floats((size_t)H * H), b_ih = read_floats(H), b_hh = read_floats(H);
    cuMatrix<float> in(x.data(), T * B, In, 1);
    in.toGpu();
    RNN rnn(B, In, H, T, 1);
    rnn.rnn_cell[0]->initParams(w_ih.data(), w_hh.data(), b_ih.data(), b_hh.data());
    print_rows(rnn.forward(&in));
    return 0;
}

// A small model with the classes' own random initialisation, end to end.
static int run_model() {
    const int B = 3, T = 9, In = 10, L = 40, H = 50, V = 4;
    Linear l1(B * T, In, L), l2(B * T, L, L), l3(B * T, L, H), l5(B * T, H, L), l6(B * T, L, V);
    RNN rnn(B, H, H, T, 1);
    cuMatrix<float> x(B * T, In, 1);
    x.toGpu();
    cuMatrix<float>* out = l6.forward(l5.forward(rnn.forward(l3.forward(l2.forward(l1.forward(&x))))));
    out->toCpu();
    if (out->getRows() != B * T || out->getCols() != V) return 1;
    for (int i = 0; i < out->getLen(); i++)
        if (!std::isfinite(out->getHost()[i])) return 1;
    printf("model %d %d\n", out->getRows(), out->getCols());
    return 0;
}

static int run_ctc(const char* vocab, int T, int B, int beam, int blank) {
    const int V = (int)strlen(vocab);
    if (run_model() != 0) {
        fprintf(stderr, "api_driver: the model's output has the wrong shape or is not finite\n");
        return 1;
    }
    std::vector<float> p = read_floats((size_t)T * B * V);
    std::vector<char> voc(vocab, vocab + V);
    CTCBeamSearch decoder(voc.data(), V, beam, blank);
    cuMatrix<float> prob(T * B, V, 1);
    memcpy(prob.getHost(), p.data(), sizeof(float) * p.size());
    prob.toGpu();
    std::vector<std::pair<std::string, float>> best = decoder.decode(&prob, T, B);
    if ((int)best.size() != B) return 1;
    for (int b = 0; b < B; b++) printf("best %s %.8g\n", best[b].first.c_str(), best[b].second);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "linear")) return run_linear(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    if (argc == 6 && !strcmp(argv[1], "rnn"))
        return run_rnn(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 7 && !strcmp(argv[1], "ctc"))
        return run_ctc(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    fprintf(stderr, "usage: api_driver linear M K N | rnn T B In H | ctc VOCAB T B BEAM BLANK  (numbers on stdin)\n");
    return 2;
}
