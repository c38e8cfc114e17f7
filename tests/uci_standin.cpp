// A minimal UCI engine over the package's own chess rules (csrc/chess_rules.h), built for the host by tests/test_gpu_chess.py: the opponent of
// the chess env tests wherever the engine built from the reference sources (oracle/_ref/stockfish) is not present.  It speaks the part of UCI
// the env's client sends (uci, setoption, isready, position fen <fen> [moves ...], go ..., quit) and answers `go` with a legal move drawn from a
// fixed-seed stream: an opponent that plays legal chess, not a strong one.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../lmrl-gym_amd/csrc/chess_rules.h"

using namespace lmrl_chess;

int main() {
    static char line[1 << 16];
    static Pos pos;
    bool have = false;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\r\n")] = 0;
        if (!strcmp(line, "uci")) {
            printf("id name uci-standin\nuciok\n");
        } else if (!strcmp(line, "isready")) {
            printf("readyok\n");
        } else if (!strcmp(line, "quit")) {
            break;
        } else if (!strncmp(line, "position fen ", 13)) {
            char *moves = strstr(line, " moves ");
            if (moves) *moves = 0;
            have = parse_fen(line + 13, pos);
            for (char *t = moves ? strtok(moves + 7, " ") : nullptr; have && t; t = strtok(nullptr, " ")) {
                char san_out[64];
                float reward;
                int done;
                have = opponent_half_step(pos, t, (int)strlen(t), san_out, &reward, &done);
            }
        } else if (!strncmp(line, "go", 2)) {
            Move mv[kMaxMoves];
            const int k = have ? gen_legal(pos, mv) : 0;
            char u[8] = "(none)";
            if (k > 0) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                uci(mv[(state >> 33) % (uint64_t)k], u);
            }
            printf("bestmove %s\n", u);
        }
    }
    return 0;
}
