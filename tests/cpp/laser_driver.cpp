// Runs three frames of examples/laser_step.cpp (solve against the resident sub-map, insertion at the optimised pose) and checks
// the life cycle the example's sub-maps must be in after them.  Prints one JSON line; exit status 0 only when every check holds.
#define LASER_STEP_NO_MAIN
#include "../../examples/laser_step.cpp"

int main() {
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    laser_step::Summary s;
    const int rc = laser_step::run(3, ba, s);
    visfs_ba_destroy(ba);
    const bool ok = rc == 0 && s.frames == 3 && s.solved == 2 && s.submaps == 1 && s.front_range_data == 6 && s.last_chi2 > 0.0 && s.max_err < 0.3;
    std::printf("{\"ok\": %s, \"frames\": %d, \"solved\": %d, \"submaps\": %d, \"front_range_data\": %d, \"last_chi2\": %.6g, \"max_err_m\": %.4g}\n",
                ok ? "true" : "false", s.frames, s.solved, s.submaps, s.front_range_data, s.last_chi2, s.max_err);
    return ok ? 0 : 1;
}
