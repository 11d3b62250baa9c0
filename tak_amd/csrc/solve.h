// solve.h — what solve.hip (host) and solve_kernels.hip (device) share: the forced-win solver behind tg_solve / tg_search_solve
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tg {

// One chunk of K positions on the device.  A work item is one (position, root move): item = offsets[pos] + ordinal of the move.
struct SolveDev {
    const uint8_t* states;   // [K][state bytes]
    const uint8_t* active;   // [K] or null: a caller's mask (tg_search_solve)
    const uint8_t* alive;    // [K] or null: SearchDev.alive of the same games
    int K, n;
    uint32_t all_moves;      // TG_SOLVE_ALL_MOVES
    uint32_t budget;         // positions one item may create in one level
    // per position
    int32_t* counts;         // legal moves (0: finished, masked or dead)
    int32_t* offsets;        // [K + 1] exclusive scan of min(counts, TG_MAX_MOVES): first item of the position, then the item total
    uint16_t* moves;         // [K][TG_MAX_MOVES], zero past counts
    int8_t* move_values;     // [K][TG_MAX_MOVES], zero past counts
    int8_t* value;
    uint16_t* best;
    uint8_t* decided;        // value != 0 after the last fold: without all_moves the later levels skip the position
    uint8_t* budget_hit;
    unsigned long long* nodes;
    // per item
    unsigned long long* item_nodes;  // positions created by ws_play, all levels
    uint8_t* item_flag;      // ITEM_ENDED | ITEM_GAVE_UP
};
// ITEM_ENDED: the root move ends the game and proves nothing for either side, so nothing is left to prove (a draw; under
// TG_SOLVE_ROAD_ONLY also flats of either colour).  ITEM_GAVE_UP: a level ran out of budget.
enum : uint8_t { ITEM_ENDED = 1, ITEM_GAVE_UP = 2 };

void launch_solve_root(hipStream_t st, const SolveDev& D);
void launch_solve_scan(hipStream_t st, const SolveDev& D);
// level L = 1 … TG_SOLVE_MAX_DEPTH over `items` work items, then the fold of every position.  `road` (TG_SOLVE_ROAD_ONLY) picks
// the ROAD instantiation: a template argument and not a field of SolveDev, which no kernel would read and which would move the
// kernel arguments of the default mode.
void launch_solve_level(hipStream_t st, const SolveDev& D, bool road, int level, int items);
void launch_solve_fold(hipStream_t st, const SolveDev& D);

}  // namespace tg
