/*
 * descriptor_body.inc -- TEST INFRASTRUCTURE ONLY.
 *
 * compute_descriptor (src/lib.rs:785-990) written once over a real type and
 * included twice by sift_oracle.c:
 *
 *   REAL float,  DESC_F32 1: desc_core_f32 -- the restatement that
 *       oracle_compute_descriptor rounds to bytes (f32 everywhere, the
 *       sample angle through an f64 atan2 and fmod, as the reference);
 *   REAL double, DESC_F32 0: desc_core_f64 -- the same expressions with every
 *       operation after the f32 inputs in double (oracle_compute_descriptor_f64).
 *
 * Writes flat[j] * norm for the 128 bins, before rounding and the 255
 * saturation.  R(c) is the literal c in REAL; RF(f) the libm function f of
 * REAL (sinf / sin, ...).  The descriptor variants of oracle_set_variant
 * (WRONG ON PURPOSE) apply to the float instance only.
 */
static void DESC_CORE(const float* img, int width, int height, float xf, float yf, float scale_in,
                      float orientation_in, REAL* out) {
    const int n_hist = DESC_HIST, n_bins = DESC_BINS;
    const int variant = DESC_F32 ? (int)(g_variant & 0xffff) : 0;
    const uint64_t x = sat_usize(roundf(xf));
    const uint64_t y = sat_usize(roundf(yf));
    const REAL scale = (REAL)scale_in, orientation = (REAL)orientation_in;
    const REAL BIN_ANGLE_STEP = (REAL)DESC_BINS / R(360.0);
    const REAL hist_width = R(3.0) * scale;
    const int radius = sat_i32((float)RF(round)(R(3.0) * scale * RF(sqrt)(R(2.0)) * (REAL)(n_hist + 1) * R(0.5)));
    const REAL rad = orientation * (R(3.14159265358979323846) / R(180.0));
    const REAL sin_ori = RF(sin)(rad), cos_ori = RF(cos)(rad);
    const REAL sin_s = sin_ori / hist_width, cos_s = cos_ori / hist_width;
    const REAL wconst = (variant & VARIANT_DESC_EXP_CONST) ? R(-0.125125) : R(-2.) / (REAL)(n_hist * n_hist);
#define DESC_ADMITTED(xi, yi, col_rot, row_rot)                                                                     \
    ((row_rot) + (REAL)(n_hist / 2) > R(-0.5) && (row_rot) + (REAL)(n_hist / 2) < (REAL)n_hist + R(0.5) &&         \
     (col_rot) + (REAL)(n_hist / 2) > R(-0.5) && (col_rot) + (REAL)(n_hist / 2) < (REAL)n_hist + R(0.5) &&         \
     (int32_t)y + (yi) > 0 && (int32_t)y + (yi) < height - 1 && (int32_t)x + (xi) > 0 && (int32_t)x + (xi) < width - 1)
    int last_yi = 0, last_xi = 0, have_last = 0;
    if (variant & VARIANT_DESC_LOST_SAMPLE) {
        for (int yi = -radius; yi <= radius; yi++)
            for (int xi = -radius; xi <= radius; xi++) {
                const REAL col_rot = (REAL)xi * cos_s - (REAL)yi * sin_s;
                const REAL row_rot = (REAL)xi * sin_s + (REAL)yi * cos_s;
                if (DESC_ADMITTED(xi, yi, col_rot, row_rot)) {
                    last_yi = yi;
                    last_xi = xi;
                    have_last = 1;
                }
            }
    }
    REAL hist[6][6][DESC_BINS];
    memset(hist, 0, sizeof(hist));
    for (int yi = -radius; yi <= radius; yi++) {
        for (int xi = -radius; xi <= radius; xi++) {
            const REAL col_rot = (REAL)xi * cos_s - (REAL)yi * sin_s;
            const REAL row_rot = (REAL)xi * sin_s + (REAL)yi * cos_s;
            REAL row_bin = row_rot + (REAL)(n_hist / 2);
            REAL col_bin = col_rot + (REAL)(n_hist / 2);
            const int32_t ay = (int32_t)y + yi;
            const int32_t ax = (int32_t)x + xi;
            if (!DESC_ADMITTED(xi, yi, col_rot, row_rot)) continue;
            if (have_last && yi == last_yi && xi == last_xi) continue; /* wrong on purpose */
            const float* r = img + (size_t)ay * width;
            const REAL dx = (REAL)r[ax + 1] - (REAL)r[ax - 1];
            const REAL dy = (REAL)img[(size_t)(ay - 1) * width + ax] - (REAL)img[(size_t)(ay + 1) * width + ax];
            const REAL wsq = col_rot * col_rot + row_rot * row_rot;
            const REAL weight = RF(exp)(wsq * wconst);
            const double deg = atan2((double)dy, (double)dx) * (180.0 / 3.14159265358979323846);
            const REAL ori = (REAL)fmod(deg + 360.0, 360.0) - orientation;
            REAL mag = RF(sqrt)(dx * dx + dy * dy);
            if ((variant & VARIANT_DESC_MAG_HALF) && yi > 0) mag *= R(1.0005); /* wrong on purpose */
            row_bin = row_bin - R(0.5);
            col_bin = col_bin - R(0.5);
            mag = mag * weight;
            REAL obin = ori * BIN_ANGLE_STEP;
            if (variant & VARIANT_DESC_ORI_BIAS) obin = obin + R(1e-4); /* wrong on purpose */
            const REAL row_floor = RF(floor)(row_bin), col_floor = RF(floor)(col_bin), ori_floor = RF(floor)(obin);
            const REAL row_frac = row_bin - row_floor, col_frac = col_bin - col_floor, ori_frac = obin - ori_floor;
            const REAL c1 = mag * row_frac, c0 = mag - c1;
            const REAL c11 = c1 * col_frac, c10 = c1 - c11;
            const REAL c01 = c0 * col_frac, c00 = c0 - c01;
            const REAL c111 = c11 * ori_frac, c110 = c11 - c111;
            const REAL c101 = c10 * ori_frac, c100 = c10 - c101;
            const REAL c011 = c01 * ori_frac, c010 = c01 - c011;
            const REAL c001 = c00 * ori_frac, c000 = c00 - c001;
            /* small integers: exact in f32 */
            const uint64_t r1 = sat_usize((float)(row_floor + R(1.))), cc1 = sat_usize((float)(col_floor + R(1.)));
            const uint64_t r2 = sat_usize((float)(row_floor + R(2.))), cc2 = sat_usize((float)(col_floor + R(2.)));
            REAL of = ori_floor;
            if (of < R(0.))
                of = of + (REAL)n_bins;
            else if (of >= (REAL)n_bins)
                of = of - (REAL)n_bins;
            const uint64_t o0 = sat_usize((float)of);
            const uint64_t o1 = o0 + 1 >= (uint64_t)n_bins ? 0 : o0 + 1;
            const int no_wrap = (variant & VARIANT_DESC_NO_WRAP) && o0 == 7; /* wrong on purpose */
            hist[r1][cc1][o0] += c000;
            hist[r1][cc2][o0] += c010;
            hist[r2][cc1][o0] += c100;
            hist[r2][cc2][o0] += c110;
            if (no_wrap) continue;
            hist[r1][cc1][o1] += c001;
            hist[r1][cc2][o1] += c011;
            hist[r2][cc1][o1] += c101;
            hist[r2][cc2][o1] += c111;
        }
    }
#undef DESC_ADMITTED
    REAL flat[DESC_SIZE];
    int i = 0;
    for (int r = 1; r < 5; r++)
        for (int c = 1; c < 5; c++)
            for (int o = 0; o < n_bins; o++) flat[i++] = hist[r][c][o];
    REAL l2 = R(0.0);
    for (int ch = 0; ch < DESC_SIZE / 4; ch++) {
        REAL s = R(0.0);
        for (int j = 0; j < 4; j++) s += flat[4 * ch + j] * flat[4 * ch + j];
        l2 = ch == 0 ? s : l2 + s;
    }
    l2 = RF(sqrt)(l2);
    const REAL cap = l2 * R(0.2);
    for (int j = 0; j < DESC_SIZE; j++) flat[j] = RF(fmin)(flat[j], cap);
    REAL l2c = R(0.0);
    for (int ch = 0; ch < DESC_SIZE / 4; ch++) {
        REAL s = R(0.0);
        for (int j = 0; j < 4; j++) s += flat[4 * ch + j] * flat[4 * ch + j];
        l2c = ch == 0 ? s : l2c + s;
    }
    l2c = RF(sqrt)(l2c);
    const REAL norm = R(512.0) / RF(fmax)(l2c, (REAL)FLT_EPSILON);
    for (int j = 0; j < DESC_SIZE; j++) out[j] = flat[j] * norm;
}
