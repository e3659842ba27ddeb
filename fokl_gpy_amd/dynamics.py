"""
Simulate a dynamic system whose right-hand sides are fitted models, for every posterior draw at once, on the device.

``simulate(models, states, inputs, forcing, y0, t, ...)`` integrates d(states[k])/dt = models[k](its inputs) with the
classical Runge-Kutta scheme, one trajectory ("member") per posterior draw and / or initial state, and returns the mean
and the order-statistic band over the members.  It is to ``GP_Integrate_ensemble`` what ``optimize_system`` is to
``optimize``: the fitted models as they are, wired by variable names.

  * either kernel, also mixed in one system; a cubic-spline model is evaluated on the fit's own 499 pieces (FR:570-589),
    so a trajectory is a trajectory of what ``evaluate`` returns;
  * ``inputs[k]`` names model k's input columns in the order of its ``mtx`` columns: states and forcing keys, any order,
    any subset;
  * states, ``y0``, forcing and ``bounds`` are in true scale; every model normalises each of its inputs with its own
    ``minmax`` row of that column;
  * a member that runs into the edge of the training range is clamped as in the reference (GI:204-269), and
    ``first_saturation`` says at which step that first happened.

``GP_Integrate`` and ``GP_Integrate_ensemble`` stay what they are: the reference's integrator, statement for statement.

The arithmetic (``simulate_host`` is its statement in numpy, the device kernel follows it operation for operation; only
+ - * /, ceil and comparisons, nothing fused, so the two agree bit for bit):

  normalisation   v = (x - lo) / (hi - lo); v > 1 -> 1; v < 0 -> 0                       (lo, hi: the model's minmax row)
  spline order o  p = ceil(499 v); p += (p == 0); p -= 1; s = 499 v - p; c0 + s (c1 + s (c2 + s c3)) of piece p
  Bernoulli o     Horner over phis[o - 1][0 .. o], highest coefficient first
  term            the product of its factors in column order
  model           0 + betas[1] term_1 + betas[2] term_2 + ... (top to bottom), then + betas[0], then * h
  slope rule      the stage's slope of state k is set to zero where the stage point is >= the box's upper edge and the
                  slope is > 0, or <= the lower edge and the slope is < 0
  step            stage points y, y + d1 / 2, y + d2 / 2, y + d3; y += (((d1 + 2 d2) + 2 d3) + d4) / 6
  forcing         row s of every forcing array serves the four stages of step s (zero-order hold, GI:187)

Step s takes point s of ``t`` to point s + 1.  ``first_saturation[e]`` is the first s in which, for member e, a
normalised input (a state's or a forcing value's) was clamped or the slope rule changed a slope; -1 if none did.

``simulate_adaptive(..., rtol=1e-6, atol=None, min_halvings=0, max_halvings=10)`` integrates the same system on the same
output grid with an error statement per member: inside every output step a member takes as many substeps of the scheme above
as ITS fitted model needs, chosen by step doubling on a dyadic grid.  ``simulate_adaptive_host`` is its statement in numpy;
only + - * /, ceil, comparisons and integer bookkeeping, in fixed orders (no pow, no sqrt), so the device agrees bit for bit.

Per member, carried over the whole run: the state y and the level k (it starts at ``min_halvings``).  With K =
``max_halvings`` and FULL = 2^K, output step s takes point s of ``t`` to point s + 1:

  1. forcing      row s serves the whole step (zero-order hold); the forcing factors are formed once, as ``simulate`` forms
                  them; a forcing clamp counts for ``first_saturation``.  pos = 0
  2. while pos < FULL:
       substep    g = h 2^-(k + 1) (an exact scaling of h)
       full       y1 = one step of ``simulate``'s scheme from y with 2 g in the place of h (stage, clamps, the slope rule on
                  the scaled slope and the sum (((d1 + 2 d2) + 2 d3) + d4) / 6 unchanged)
       halves     ya = one such step from y with g; y2 = one such step from ya with g
       estimate   per state j in order, |.| and max by comparison: d_j = |y2_j - y1_j|,
                  sc_j = atol_j + rtol max(|y_j|, |y2_j|)
       ok         d_j <= 15 sc_j for every j: the Richardson estimate d / 15 of y2's local error within tolerance
       easy       64 d_j <= 15 sc_j for every j: a step twice as long has 32 times the local error, and a factor 2 of safety
                  (a NaN fails both tests)
       accept     if ok or k == K: y = y2; pos += FULL >> k; pairs += 1; if not ok the step is forced and
                  ``first_unresolved`` takes s if it is still -1; if a clamp or the slope rule acted in either half step
                  ``first_saturation`` takes s if it is still -1; error = r where r > error, r = max_j d_j / (15 sc_j) formed
                  from 0.0 by r = q where q > r (a NaN is never taken); levels[s] = max(levels[s], k); max_level likewise.
                  Then, if easy and k > min_halvings and pos mod 2^(K - k + 1) == 0: k -= 1 (pos == FULL is aligned, so a
                  level can relax at the end of a step)
       reject     otherwise: k += 1; rejected += 1
  3. point s + 1 is y

Every iteration advances pos or raises k, and k cannot pass K: the loop ends for any input, NaN coefficients included.  pos
stays a multiple of FULL >> k, so a pair never crosses an output point.  y2 is accepted as it is (no local extrapolation).
With ``min_halvings`` = ``max_halvings`` = L every member takes pairs of half steps of h / 2^(L + 1) throughout: the members
equal ``simulate_host``'s on the grid (start, stop, h / 2^(L + 1)) with every forcing row repeated 2^(L + 1) times, at every
2^(L + 1)-th point, bit for bit, and ``first_saturation`` equals that run's integer-divided by 2^(L + 1).  A member that meets
the wall of the box sits on a kink of the right-hand side, which no step size resolves: ``first_unresolved`` says so.

``simulate_stiff(..., rtol=1e-4, atol=None, min_halvings=0, max_halvings=10)`` is the linearly implicit sibling for members
whose fitted model is stiff: Rodas3 (four stages, order 3 with an embedded order 2, gamma = 1 / 2, A- and L-stable) under the
same per-member dyadic controller, so a decayed fast mode no longer chooses the step.  ``simulate_stiff_host`` is its statement
in numpy; only + - * /, ceil, comparisons and integer bookkeeping, in fixed orders, so the device agrees bit for bit.  On
dy/dt = b (y - y*) a step of size g multiplies y - y* by R(z) = 8 (z^3 - 6 z + 6) / (3 (z - 2)^4), z = b g.

Per member, carried over the whole run: y and the level k (from ``min_halvings``).  Output step s, K = ``max_halvings``,
FULL = 2^K; the forcing factors of row s are formed once as above (the system is autonomous inside the step), pos = 0:

  while pos < FULL:
    step size     g = h 2^-k (an exact scaling); c2 = 2.0 / g, c4 = 4.0 / g, ig = 1.0 / g, c83 = 8.0 / 3.0
    F(x)          the stage above with a step of 1: clamps, the model, the slope rule on the unscaled slope
    F0, J         F(y) and J[r][d] = d F_r / d y_d by ``control``'s tangent rules, one direction d at a time: the input of
                  state j has tangent (1.0 if j == d else 0.0) / span, 0 where its clamp acted; a factor's tangent is its
                  slope (``_factor_dual``) times its input's tangent, a forcing factor's is 0; a term's
                  t_phi = t_phi fac + phi t_fac over its slots in order (from 1, 0); t_delta = t_delta + beta t_phi; row r of
                  J is 0 where the slope rule acted on state r
    W             W[r][r] = c2 - J[r][r]; W[r][d] = -J[r][d] elsewhere
    LU            ``stiff_lu``: for column c = 0 .. NS - 1: best = |W[c][c]|, row = c; for r = c + 1 ..: row = r and
                  best = |W[r][c]| where |W[r][c]| > best (ties and NaN keep the lower row); rows c and row are exchanged
                  from column c on (the multipliers left of it stay; the exchange is counted); then for r > c: l = W[r][c] / W[c][c], stored in W[r][c], and
                  W[r][j] = W[r][j] - l W[c][j] for j = c + 1 .. in order.  |x| is -x where x < 0
    solve(b)      ``stiff_solve``: for c = 0 ..: exchange b[c] and b[row_c]; then for r > c: b[r] = b[r] - W[r][c] b[c];
                  then for c = NS - 1 .. 0: b[c] = b[c] / W[c][c]; for r = 0 .. c - 1: b[r] = b[r] - W[r][c] b[c]
    stages        K1 = solve(F0); K2 = solve(F0 + c4 K1); y3 = y + 2.0 K1; K3 = solve(F(y3) + (K1 - K2) ig); y4 = y3 + K3;
                  K4 = solve(F(y4) + ((K1 - K2) - c83 K3) ig); y_new = y4 + K4; the estimate is K4
    test          per state j in order: e_j = |K4_j|, sc_j = atol_j + rtol max(|y_j|, |y_new_j|); ok: e_j <= sc_j for every
                  j; easy: 16.0 e_j <= sc_j for every j (the estimate falls by 8 when g halves, and a factor 2 of safety); a
                  NaN fails both; r = max_j e_j / sc_j formed from 0.0 by r = q where q > r
    accept        if ok or k == K: y = y_new; pos += FULL >> k; steps += 1; swaps += the trial's exchanges; forced (not ok)
                  sets ``first_unresolved``; a clamp or the slope rule in F(y), F(y3) or F(y4) sets ``first_saturation``;
                  error, levels[s], max_level and the relaxation of k (easy, k > min_halvings, pos aligned) as above
    reject        otherwise: k += 1; rejected += 1

A zero pivot is not special: the division gives inf or NaN, the trial fails, and at k == K the member takes the NaN as a NaN
coefficient's member does above.  Three evaluations of F, one Jacobian and one factorisation per trial.

``steady_states(models, states, inputs, at={...}, starts=9, ...)`` says where the same system comes to rest: a damped Newton
iteration on F(y) = 0 per member (operating point q, posterior draw e, start s), every member at once on the device.  F and J
are the stage and the Jacobian of ``simulate_stiff`` above with a step of 1, clamps and slope rule included, so a rest point
found here is a rest point of ``simulate``.  ``steady_states_host`` is its statement in numpy; only + - * /, ceil, comparisons
and integer bookkeeping, in fixed orders, so the device agrees bit for bit in every per-member field.

  operating point ``at`` gives every input column that is not a state, a number or [Q] values in true scale; row q is a
                  forcing row: its factors are formed once, as ``simulate`` forms them
  starts          the same S for every (q, e).  An integer S: start 0 is lo + (hi - lo) 0.5, start i >= 1 is
                  lo_j + u_ij (hi_j - lo_j) with u_ij the radical inverse of i in base 2, 3, 5, 7, 11, 13, 17, 19 for state
                  j = 0 .. 7 (r = 0, f = 1; while i > 0: f = f / base, r = r + f (i mod base), i = i div base)
  ratio(F)        r = 0.0; per state j in order: q = |F_j| / ftol_j; r = q where q > r or q != q (a NaN is taken and kept)

Per member, from y = its start, iterations = halvings = 0:

  1. evaluate     (F, J) = (F0, J) of ``simulate_stiff`` at y; r = ratio(F).  ``residual`` = r, ``jacobian`` = J and
                  ``on_wall`` = held (3.) are those of the last evaluation
  2. end          status 3 unless r < inf (r is NaN or inf); else status 0 if r <= 1; else status 1 if iterations == max_iter
  3. held         row k is held if F_k == 0 and J[k][d] == 0 for every d: a state on the wall with its slope switched off, or
                  a model that is flat there
  4. step         W[r][d] = -J[r][d]; W[k][k] = 1.0 on held rows; delta = solve(F) by ``stiff_lu`` / ``stiff_solve`` of W;
                  delta_k = 0.0 on held rows (a held state does not move)
  5. line search  for b = 0 .. max_halvings: y_t = y + delta 2^-b (an exact scaling), per state lo where y_t < lo and hi where
                  y_t > hi (a NaN stays); F_t = F(y_t) by the value operations alone; r_t = ratio(F_t); the first b with
                  r_t < r is taken (a NaN compares false) and halvings += b.  No b: status 2 (stalled), y stays,
                  halvings += max_halvings + 1
  6. accept       y = y_t; iterations += 1; go to 1

Both loops have fixed bounds (max_iter + 1 evaluations, max_halvings + 1 trial points), so a member ends for any input.  A
singular W gives inf or NaN in delta, every trial point fails its test and the member stalls; a NaN coefficient ends the
member at its first evaluation with status 3; neither touches another member.  What follows from the per-member fields is
numpy on the host, the same code after both functions: the eigenvalues of the free sub-block of J (``np.linalg.eigvals``),
``stable``, the distinct roots of every (q, e) and the summaries over the draws (``steady_states``'s docstring).

``assimilate(models, states, inputs, ..., observe, data, ...)`` filters the same system against measurements: a bootstrap
particle filter of 64 particles per posterior draw, every draw at once on the device.  It returns the filtered states
(per draw and pooled over the draws), and per draw the log marginal likelihood of the measurements, which normalised
over the draws re-weights the model's posterior without a refit.  ``assimilate_host`` is its statement in numpy.

The filter's arithmetic, per draw e with id ``draw_ids[e]`` (the selected row of ``betas``, so a subset of the draws
reproduces the full run), per particle (lane) i:

  start           y_j = y0_j + y0_sd_j normal(step 0, purpose INIT, index 64 j + i); W_i = 1 / 64
  step s          one step of ``simulate`` above, operation for operation, with the draw's coefficients (point s -> s + 1)
  process noise   y_j = y_j + q_j normal(step s + 1, purpose j, index i), q_j = process_sd_j sqrt(h) formed once; nothing
                  is drawn or added where q_j == 0
  weighting       at a point that carries row r of ``data``, over the present (not NaN) entries o in the order of ``observe``:
                  lw_i = -0.5 (0 + ((data_o - y_obs(o)) / obs_sd_o)^2 + ...); m = max_i lw_i; g_i = W_i exp(lw_i - m);
                  G = sum_i g_i; the log evidence grows by (m + log G) - sum_o log(obs_sd_o sqrt(2 pi)); W_i = g_i / G.
                  A row without a present entry changes neither weights nor evidence and does not resample
  statistics      taken there, before resampling: ESS = 1 / sum_i W_i^2, mu_j = sum_i W_i y_ij,
                  var_j = sum_i W_i ((y_ij - mu_j) (y_ij - mu_j))
  resampling      if ESS < resample_below 64: u = uniform(step = the point, purpose RESAMPLE, index 0), c = the inclusive
                  prefix sum of W, particle i takes the ancestor a_i = min(63, #{k : c_k <= (i + u) / 64 c_63}); the
                  states are gathered and W_i = 1 / 64
  collapse        if G is not a positive finite number, or m < -745 (exp(m) is no positive double: every particle is
                  impossibly far from the row) or m is NaN: the row's increment is -inf, so the draw's evidence is -inf
                  from there on; W_i = 1 / 64; ``collapsed[e]`` keeps the first such row.  No other draw is touched
  saturation      ``first_saturation[e]`` is the first step in which a clamp or the slope rule acted for any particle of e

Sums and maxima over the 64 lanes are the xor butterfly with offsets 32, 16, 8, 4, 2, 1: lane i combines its value with
lane i ^ offset's (``lane_sum``, ``lane_max``; the maximum is fmax, which passes over a NaN).  The prefix sum is the
Hillis-Steele scan with offsets 1, 2, 4, 8, 16, 32: c_i += c_(i - offset) for i >= offset (``lane_scan``).  The random
numbers are Philox 4x32-10 (csrc/fokl_philox.h) with key (seed, draw id) and counter (step, purpose, index, 2), drawn
on the host through ``_capi.assimilate_rng``; normals are Box-Muller, one per counter.  Without noise a particle is
``simulate_host``'s member bit for bit; weights, evidence and normals pass through exp / log / cos and agree between the
device and this host to the two maths libraries' last bits.

Pooling over the draws at observation k: draw e weighs exp(log_evidence[e, k]) normalised over the draws (uniform if all
are -inf); ``mean`` is the weighted mean of ``draw_mean``, ``sd`` the root of the weighted within-draw variance plus
the weighted squared distance of ``draw_mean`` to ``mean``.

``calibrate(models, states, inputs, ..., unknown=['y0:c', 'k'], observe, data, ...)`` answers what comes before filtering and
control: a run of the plant was measured; which initial state and which constant operating inputs produced it?  One
affine-invariant ensemble sampler (``infer.py``'s: stretch moves, a differential-evolution jump every few iterations,
counter-based Philox numbers) of W = 128 walkers over the d unknowns per posterior draw, every draw at once on the device, so
the answer carries the model's own uncertainty.  ``calibrate_host`` is its statement in numpy, not a fallback.

  unknowns        ``'y0:<state>'`` is that state's initial value, its box the state's box; any other name is a parameter: an
                  input column that is neither a state nor a key of ``forcing`` (``control``'s rule for ``controls``),
                  constant over the run and per walker.  It passes through ``_prepare`` as a placeholder forcing column;
                  ``norm_param[n]`` is the unknown forcing input n reads, -1 for a real forcing column.  A parameter's box
                  is the intersection of the training ranges of the columns that read it; ``unknown_bounds`` may narrow a
                  box and may not leave it.  1 <= d <= 16.  theta is in true scale throughout
  trajectory      for draw e and walker theta: ``simulate``'s, operation for operation, with the draw's coefficients, y0
                  overwritten in the unknown states, and every parameter held at its value: the normalised value of a
                  parameter is clamp((theta - lo_n) / span_n) per reading column n, exactly as a forcing value.  The
                  factors that read a parameter are formed once per trajectory, those of a real forcing column once per
                  step
  target          ss = 0; over the observed points in ascending order (point 0 may be observed) and the observed columns in
                  ascending order, where ``data`` is not NaN: r = data - y; ss = ss + hp_o (r r), hp_o = 0.5 / obs_sd_o^2
                  formed once; pp = 0; for i = 0 .. d - 1: dl = theta_i - mean_i; pp = pp + prec_i (dl dl), prec_i =
                  1 / sd_i^2 formed once (0: no prior beyond the box); lp = -ss - 0.5 pp.  Outside the open box
                  lo < theta < hi lp = -inf and nothing is integrated.  Only + - * /, ceil and comparisons: lp is the
                  device's bit for bit.  ``saturated``: a clamp or the slope rule acted somewhere along the trajectory
  starts          ``optimize.start_points(128, lo, hi)``, the same for every draw, or user ``starts`` [128, d] strictly
                  inside the box
  iteration t     t = 0, 1, ... (burn-in included) updates half 0 (walkers 0 .. 63), then half 1 (64 .. 127); a moving
                  walker w of half hf reads the OTHER half as it stands at that moment (half 1 sees half 0 already moved).
                  With the uniforms u1, u2, u3 of walker w at iteration t:
    stretch       j = 64 (1 - hf) + floor(64 u1); z = (1 + u2)^2 / 2; y = x_j + z (x_w - x_j);
                  log_ratio = (d - 1) log z + lp(y) - lp(x_w)
    jump          when jump_every > 0 and t % jump_every == jump_every - 1: a = floor(64 u1),
                  b = (a + 1 + floor(63 u2)) mod 64, both in the other half; y_i = (x_w,i + (x_a,i - x_b,i)) +
                  (1e-5 (hi_i - lo_i)) n_i; log_ratio = lp(y) - lp(x_w)
    acceptance    a proposal outside the box is rejected without an evaluation; otherwise it is accepted iff
                  log(u3) < log_ratio.  A walker whose lp is NaN is never left and never copied by an accept (both
                  comparisons are false); ``invalid[e]`` says that a start of draw e had no finite lp, and no other draw
                  is touched
  random numbers  Philox 4x32-10, key (seed, the draw's row of ``betas``), counter (t, purpose, index, 3); purposes 0, 1, 2
                  are u1, u2, u3 with index = walker 0 .. 127, purpose 3 the jitter normal n_i (Box-Muller) with index
                  128 i + w; the host reads them through ``_capi.calibrate_rng``
  kept            row r is the state after both halves of iteration burnin + r thin, r < ceil(draws_kept / thin); per
                  walker and half of the ``draws_kept`` post-burn-in iterations (the first draws_kept // 2, then the rest)
                  the sum and the sum of squares of theta_i - (lo_i + hi_i) / 2 in iteration order (split R-hat over 256
                  chains); per walker the accepted stretch and jump moves; per draw the trajectories integrated

No transcendental enters a stretch proposal or lp; log z, log u3 and the jump's normal pass through log / cos and agree
between the device and this host to the two maths libraries' last bits, which can flip an acceptance: compare flags, and
states where the flags agree.  Counter-based numbers make draw e alone the draw e of the full run, and a thin = 3 run's rows
every third row of the thin = 1 run, bit for bit.  LDS bytes of the kernel: (1 + factors + normalised states + 7 d) x 64 x
8 + coefficients x 8, at most 144 KB (``calibrate_lds_bytes``).

``control(models, states, inputs, controls=[...], ..., targets, limits, move_weight, ...)`` answers what such a system is
fitted for: which inputs, held piecewise constant over the coming horizon, make the states do what is wanted -- one bounded
least-squares solve per posterior draw and start, every solve at once on the device, so the answer comes with its
uncertainty as ``optimize``'s does.  ``control_host`` is its statement in numpy.  ``assimilate`` returns what a controller
starts from (``draw_mean[:, :, -1]`` as ``y0`` [E, n_states], ``draw_index`` as ``draws=``), so the loop assimilate ->
control -> apply -> assimilate closes inside the package.

The cost is a sum of weighted squares of residuals a - b, listed by point: with y the trajectory of ``simulate``'s scheme
(clamps and slope rule included) under u_ck = lo_c + z_ck (hi_c - lo_c), control c on segment k, decision value d = c K + k,

  at point p = 1 .. P - 1, per state j in order:
      tracking    weight h w_j,          y_j(p) - ref_j(p)         where w_j > 0 and ref_j(p) is not NaN
      terminal    weight terminal_j,     y_j(P - 1) - ref_j(P - 1) at the last point, where terminal_j > 0
      upper limit weight h limit_weight, y_j(p) - hi_j             where y_j(p) > hi_j (otherwise it adds nothing)
      lower limit weight h limit_weight, lo_j - y_j(p)             where y_j(p) < lo_j
  then per control c, per segment k (k = 0 only with ``previous``):
      move        weight move_c,         u_ck - u_c,k-1            (u_c,-1 = previous_c)

  F = sum weight (a - b)^2 accumulated as F = F + (weight r) r; S = sum weight (|a| + |b|)^2 is the rounding scale of F.

One solve, operation for operation (only + - * /, sqrt, ceil and comparisons, in fixed orders, nothing fused):

  1. Tangent pass.  Direction d (a lane of the wavefront) carries, next to every value of ``simulate``'s step, its
     derivative with respect to z_d:
       a controlled column   v = ((lo_c + z_ck (hi_c - lo_c)) - lo) / span, clamped as any input; t_v = (hi_c - lo_c) / span
                             for d = c K + k (k the segment of the step), else 0; a state's input has t_v = t_y / span;
                             a clamp that acts (v > 1 or v < 0; a value exactly on 0 or 1 is not clamped) sets t_v = 0
       Bernoulli factor      value = c_o, slope = 0; for k = o - 1 .. 0: slope = slope v + value; value = value v + c_k
       spline factor         the value's piece and s: q2 = c2 + s c3; q1 = c1 + s q2; value = c0 + s q1; d1 = q2 + s c3;
                             d0 = q1 + s d1; slope = 499 d0
       factor tangent        slope t_v
       term                  over its entry's slots in order: t_phi = t_phi fac + phi t_fac; phi = phi fac (from 1, 0)
       model                 delta = delta + beta phi, t_delta = t_delta + beta t_phi; the slope (delta + beta_0) h has
                             tangent t_delta h; a slope the slope rule zeroes has tangent 0
       step                  the stage points and the sum of the stages carry their tangents through the same formulas
     Per residual with tangent t (of y_j: t_y; of lo_j - y_j: -t_y; of a move: hi_c - lo_c in d = c K + k, -(hi_c - lo_c)
     in d - 1): g_d = g_d + (2 (weight r)) t_d and H[d][d'] = H[d][d'] + ((2 weight) t_d) t_d'.  So g = 2 J' r, H = 2 J' J,
     the derivative of the scheme as executed.
  2. Stop test: non-finite F or g ends the solve (status 2); max_d |P(z - g)_d - z_d| <= tol ends it converged (0), P the
     clip to [0, 1] by comparisons; iteration ``max_iter`` ends it at the limit (1).  (``optimize``'s codes.)
  3. Active set: coordinate d is active where z_d <= 0 and g_d > 0, or z_d >= 1 and g_d < 0.
  4. Modified Cholesky of the lower triangle, column by column, row i >= j: s = H[i][j] (1 on the diagonal and 0 off it
     where i or j is active) - L[i][0] L[j][0] - ... - L[i][j-1] L[j][j-1]; the pivot s is replaced by max(|s|, floor)
     unless s > floor = 1e-8 max(1, largest |H[d][d]| over the free d); L[j][j] = sqrt(s), L[i][j] = s / L[j][j].  Forward
     substitution from -g (0 where active) for k = 0 .. D - 1: s_k = s_k / L[k][k], then s_i = s_i - L[i][k] s_k for i > k;
     back substitution for k = D - 1 .. 0: s_k = s_k / L[k][k], then s_i = s_i - L[k][i] s_k for i < k.
  5. Arc search, every trial point in one pass: lane i < 31 tries P(z + 2^-i d), lane 32 + i tries P(z + 2^-i (-g)).  A
     lane passes if its point moves z (some |step_d| > 0) and F_trial <= (F + 1e-4 min(slope, 0)) + 1e-13 S with
     slope = g_0 step_0 + g_1 step_1 + ... in order.  The first passing Newton lane is taken, else the first passing
     steepest-descent lane, else the solve ends stalled (3).  The trial F is formed by the value operations above alone.

One iteration is one tangent pass and one trial pass.  The returned cost is F of the tangent pass at the returned point; the
best start of a draw has the smallest finite cost; every draw's trajectory under its own controls (``mean``, ``bounds``,
``members``, ``first_saturation``) is ``simulate_host``'s under ``expand_controls(res, e)``, bit for bit.  The device follows
the statement operation for operation: the tangent pass agrees bit for bit, whole solves in status, iterations and 1e-9.

``control_pooled(..., draw_weights=None, ...)`` finds ONE control sequence for the whole posterior: it minimises the expected
cost F(z) = sum_e w_e F_e(z) over the one decision vector z, F_e being exactly ``control``'s cost of draw e and w the
normalised draw weights (uniform, or for example ``assimilate``'s ``weights``).  A weighted sum of sums of squares is a sum
of squares again, so projected Gauss-Newton stays exact with g = sum_e w_e g_e and H = sum_e w_e H_e; there is one solve per
start, not per (draw, start).  ``control_pooled_host`` is its statement in numpy.

  pooled sum      ``pooled_sum(X, w)``, used for F, S (the rounding scale), g, H and the trial costs alike: the draws are cut
                  into chunks of ``POOL_CHUNK`` = 64 consecutive indices; inside a chunk acc = acc + w_e X_e runs in index
                  order from 0.0; the chunk sums are then added in chunk order from the first.  A draw with w_e == 0 is
                  skipped entirely (no multiply, no add), so a collapsed draw of ``assimilate`` (weight 0, possibly NaN
                  states) cannot poison the sum.  Only + and *, in an order no launch shape changes: the device reproduces
                  it bit for bit
  one iteration   steps 1 .. 5 of ``control`` with the pooled F, S, g, H in place of one draw's: the tangent pass of every
                  draw at the shared z, the pooled sum, the same stop test (a non-finite pooled F or g: status 2), active
                  set, modified Cholesky and 31 + 31 trial points, the value pass of every draw at every trial point, the
                  pooled sum of the trial costs, the same Armijo test, the first passing lane

The returned cost is the pooled F of the tangent pass at the returned point, ``cost_draws`` the draws' own costs there
(cost == pooled_sum(cost_draws, w)); every draw's trajectory under the shared controls is ``simulate_host``'s under
``expand_controls(res)``, bit for bit.  With one draw the solve is ``control``'s, bit for bit (0.0 + 1.0 X is X).

``control_cvar(..., alpha=0.9, smoothing=0.01, epsilon=None, ...)`` finds ONE control sequence that protects the bad tail of
the posterior: in place of the expected cost it minimises the smoothed conditional value at risk at level alpha of the
draws' costs (Rockafellar and Uryasev), with m = 1 - alpha and live draws those with w_e != 0,

    phi(z) = min_a  a + (1 / m) sum_e w_e s_eps(F_e(z) - a),
    s_eps(t) = 0 for t <= 0,  t^2 / (2 eps) for 0 < t < eps,  t - eps / 2 for t >= eps        (C1)

so cvar - eps / (2 m) <= phi <= cvar.  ``control_cvar_host`` is its statement in numpy; ``cvar_smooth`` is the risk and
``cvar_exact`` the exact CVaR that is reported.  alpha = 0 IS ``control_pooled`` (q = w, no a, no covariance term), bit for bit.

  finding a       64 bisections, nothing else: lo = min_e F_e - eps and hi = max_e F_e over the live draws; each step
                  mid = lo + 0.5 (hi - lo), h = pooled_sum(clip((F - mid) / eps, 0, 1), w), lo = mid if h > m, else hi = mid;
                  a = hi.  The clip is two comparisons
  soft weights    r_e = clip((F_e - a) / eps, 0, 1); q_e = (w_e r_e) / m (they sum to 1 up to the bisection's resolution);
                  c_e = w_e / (m eps) where 0 < F_e - a < eps, else 0; a draw of weight 0 has q_e = c_e = 0
  pooled values   phi = a + pooled_sum(s_eps(F - a), w) / m with s_eps's middle piece as (t t) / (2 eps) and its last as
                  t - 0.5 eps; S = pooled_sum(S_e, q); g = pooled_sum(g_e, q);
                  H = pooled_sum(H_e, q) + [Scgg - (Scg Scg') / Sc] with Sc = pooled_sum(1, c), Scg = pooled_sum(g_e, c),
                  Scgg[d][d'] = pooled_sum(g_ed g_ed', c): the Schur complement of a, the band draws' covariance of gradients
                  (positive semi-definite), dropped where Sc == 0.  A draw with q_e == 0 (c_e == 0) is skipped in the q-sums
                  (c-sums), as a draw of weight 0 is.  A live draw with a non-finite F_e makes phi and a NaN and q = c = 0: at z
                  that is status 2, and a trial lane with such a draw fails its test
  one iteration   ``control_pooled``'s with phi, S, g, H in place of the pooled F, S, g, H: the same stop test, active set,
                  modified Cholesky, 31 + 31 trial points, Armijo test (on phi of each trial lane, found with the same
                  bisection per lane), first passing lane, status codes and best start
  eps             ``epsilon`` in cost units, or ``smoothing`` x pooled_sum(F_e(z0 of start 0), w); fixed for the whole call and
                  all starts, so the starts' costs stay comparable

The returned cost is phi of the tangent pass at the returned point; cvar, var, expected_cost, tail_weights and a are formed
from ``cost_draws`` by ``cvar_exact``, ``pooled_sum`` and ``cvar_smooth``.  Ranking the draws and descending on the
tail-weighted sum instead (the subgradient route) zigzags across the kinks where draws enter and leave the tail and ends at
the iteration limit; without the covariance term the smooth iteration does too.
"""
import numpy as np

from . import _capi
from . import getKernels
from .GP_Integrate import bounds_cut, _device_context
from .optimize import _model_fields

MAX_STATES = 8
MAX_BAND_MEMBERS = 16384
LANES = 64
LDS_BUDGET = 144 * 1024                   # bytes of LDS a wavefront of the kernel may ask for
LDS_ROWS = LDS_BUDGET // (LANES * 8)      # values per member: 1 + factors + normalised states + coefficients
PIECES = getKernels.N_PIECE
SPLINE, BERNOULLI = getKernels.KERNEL_SPLINES, getKernels.KERNEL_BERNOULLI
BERNOULLI_WIDTH = 21                      # coefficients of the highest shipped order (20)


class SimulateResult(dict):
    """A dict whose entries are also attributes (``res.mean``, ``res['mean']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


# ---------------------------------------------------------------------------------------------------------
# the two basis functions as the integrator evaluates them
# ---------------------------------------------------------------------------------------------------------

def spline_value(pieces, v):
    """One cubic-spline basis at normalised v (array): ``pieces`` [499, 4] holds c0 .. c3 of every piece."""
    v = np.asarray(v, dtype=np.float64)
    p = np.ceil(v * 499.0)
    p = p + (p == 0)
    p = p - 1
    s = 499.0 * v - p
    index = np.clip(np.where(np.isfinite(p), p, 0.0), 0, PIECES - 1).astype(np.intp)   # (a NaN reads piece 0, as the kernel)
    c = pieces[index]
    return c[..., 0] + s * (c[..., 1] + s * (c[..., 2] + s * c[..., 3]))


def bernoulli_value(c, v):
    """One Bernoulli basis at normalised v (array): ``c`` its coefficients, lowest power first (a row of ``phis``)."""
    v = np.asarray(v, dtype=np.float64)
    value = np.full(v.shape, float(c[len(c) - 1]))
    for k in range(len(c) - 2, -1, -1):
        value = value * v + float(c[k])
    return value


def spline_pieces(phis, order):
    """Order ``order`` (1-based) of a cubic-spline ``phis`` as [499, 4]."""
    return np.ascontiguousarray(np.stack([np.asarray(phis[order - 1][q], dtype=np.float64) for q in range(4)], axis=1))


# ---------------------------------------------------------------------------------------------------------
# checks and the plan both sides run
# ---------------------------------------------------------------------------------------------------------

def _select(betas, draws, k):
    if draws is None:
        return betas
    if isinstance(draws, str):
        if draws != 'mean':
            raise ValueError("draws must be None (all rows), an integer (the last rows), an index array or 'mean'")
        return np.mean(betas, axis=0, keepdims=True)
    if np.ndim(draws) == 0:
        if int(draws) != draws or not 1 <= int(draws) <= betas.shape[0]:
            raise ValueError(f"draws must be None (all), an integer in 1..{betas.shape[0]} (the last rows of models[{k}]'s "
                             f"betas), an index array or 'mean'")
        return betas[betas.shape[0] - int(draws):]
    index = np.asarray(draws)
    if index.ndim != 1 or index.shape[0] == 0 or not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"draws as an array must hold at least one integer index into the {betas.shape[0]} rows of betas")
    return betas[index]


def _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, lds_per_member=True):
    """Every check and every array ``_run_host`` and the device need; touches no device.  ``lds_per_member``: refuse a
    system whose values per member exceed ``simulate``'s LDS (``assimilate`` holds the coefficients once and checks its
    own need)."""
    if models is None or len(models) == 0:
        raise ValueError("simulate needs at least one fitted model (models is empty)")
    models = [_model_fields(model, k) for k, model in enumerate(models)]
    K = len(models)
    states = [str(name) for name in states]
    if len(states) != K or len(inputs) != K:
        raise ValueError(f"states and inputs need one entry per model: {K} models, {len(states)} states, {len(inputs)} input lists")
    if len(set(states)) != K:
        raise ValueError(f"states: every model integrates a state of its own, got {states}")
    if K > MAX_STATES:
        raise ValueError(f"simulate integrates at most {MAX_STATES} states, the system has {K}")
    if keep not in (None, 'members'):
        raise ValueError("keep must be None or 'members'")
    forcing = {str(name): np.asarray(values, dtype=np.float64) for name, values in dict(forcing or {}).items()}
    both = [name for name in forcing if name in states]
    if both:
        raise ValueError(f"forcing: {both} are states")

    start, stop, h = (float(v) for v in t)
    if not (np.isfinite([start, stop, h]).all() and h > 0):
        raise ValueError("t = (start, stop, h) needs finite numbers and h > 0")
    T = np.arange(start, stop + h, h)
    n_steps = len(T) - 1
    if n_steps < 0:
        raise ValueError("t = (start, stop, h) holds no point")
    for name, values in forcing.items():
        if values.ndim != 1:
            raise ValueError(f"forcing['{name}'] must be [steps]")
        if values.shape[0] < n_steps:
            raise ValueError(f"forcing['{name}'] has {values.shape[0]} values but {n_steps} steps are integrated")
        if np.isnan(values[:n_steps]).any():
            raise ValueError(f"forcing['{name}'] holds NaN")

    # ---- the models: kernel, orders, coefficients, and the normalisation of every input column ----
    state_of = {name: j for j, name in enumerate(states)}
    forcing_cols = []                                                 # forcing names some model reads, first seen first
    norms, norm_of = [], {}                                           # (source, lo, hi): source >= 0 a state, -(c + 1) forcing column c
    factors, factor_of = [], {}                                       # (norm, kind, order)
    tables = {}                                                       # (kind, order) -> coefficients
    range_lo, range_hi = np.full(K, -np.inf), np.full(K, np.inf)
    mtxs, betas, term_factors = [], [], []
    for k, model in enumerate(models):
        kernel, phis = model['kernel'], model['phis']
        if kernel in (0, 'Cubic Splines'):
            kind = SPLINE
            if len(phis) == 0 or np.ndim(phis[0][0]) != 1 or len(phis[0]) != 4 or len(phis[0][0]) != PIECES:
                raise ValueError(f"models[{k}]: a 'Cubic Splines' model needs phis of {PIECES} pieces x 4 coefficients per order")
        elif kernel in (1, 'Bernoulli Polynomials'):
            kind = BERNOULLI
            if len(phis) == 0 or np.ndim(phis[0][0]) != 0:
                raise ValueError(f"models[{k}]: a 'Bernoulli Polynomials' model needs its coefficient table in phis")
        else:
            raise ValueError(f"models[{k}]: the kernel {kernel!r} is not supported")
        mtx = np.asarray(model['mtx'])
        if mtx.ndim == 1:
            mtx = mtx[np.newaxis, :]
        if mtx.ndim != 2:
            raise ValueError(f"models[{k}]: mtx must be [terms, inputs]")
        mtx = np.ascontiguousarray(mtx, dtype=np.int32)
        names = [str(name) for name in inputs[k]]
        if len(names) != mtx.shape[1]:
            raise ValueError(f"models[{k}] has {mtx.shape[1]} input columns (mtx.shape[1]), inputs[{k}] names {len(names)}")
        for name in names:
            if name not in state_of and name not in forcing:
                raise ValueError(f"inputs[{k}]: '{name}' is neither a state ({states}) nor a forcing key ({list(forcing)})")
        if mtx.min(initial=0) < 0 or mtx.max(initial=0) > len(phis):
            raise ValueError(f"models[{k}]: mtx holds an order outside the coefficient table")
        if kind == BERNOULLI and mtx.max(initial=0) >= BERNOULLI_WIDTH:
            raise ValueError(f"models[{k}]: Bernoulli orders above {BERNOULLI_WIDTH - 1} are not handled")
        b = np.asarray(model['betas'], dtype=np.float64)
        if b.ndim == 1:
            b = b[np.newaxis, :]
        if b.ndim != 2 or b.shape[0] == 0:
            raise ValueError(f"models[{k}]: betas must be [draws, terms + 1] or [terms + 1]")
        if b.shape[1] != mtx.shape[0] + 1:
            raise ValueError(f"models[{k}]: betas has {b.shape[1]} coefficients per draw, mtx describes {mtx.shape[0]} "
                             f"terms + the constant")
        b = _select(b, draws, k)
        minmax = model['minmax']
        if len(minmax) != mtx.shape[1]:
            raise ValueError(f"models[{k}]: minmax describes {len(minmax)} inputs, mtx {mtx.shape[1]}")
        low = np.array([float(minmax[j][0]) for j in range(mtx.shape[1])])
        high = np.array([float(minmax[j][1]) for j in range(mtx.shape[1])])
        if not np.all(high - low > 0):
            raise ValueError(f"models[{k}]: minmax must have max > min for every input")
        for j, name in enumerate(names):
            if name in state_of:
                source = state_of[name]
                range_lo[source], range_hi[source] = max(range_lo[source], low[j]), min(range_hi[source], high[j])
        rows, checked = [], set()
        for i in range(mtx.shape[0]):
            row = []
            for j in range(mtx.shape[1]):
                order = int(mtx[i, j])
                if order == 0:
                    continue
                if order not in checked:                              # once per model and order
                    checked.add(order)
                    c = spline_pieces(phis, order) if kind == SPLINE else np.array(phis[order - 1][:order + 1], dtype=np.float64)
                    if kind == BERNOULLI and c.shape[0] != order + 1:
                        raise ValueError(f"models[{k}]: order {order} of its Bernoulli table has {c.shape[0]} coefficients, "
                                         f"not {order + 1}")
                    if not np.array_equal(tables.setdefault((kind, order), c), c):
                        raise ValueError(f"models[{k}]: its coefficient table (phis) differs from another model's of the "
                                         f"same kernel")
                name = names[j]                                       # a column is normalised where a factor reads it
                if name in state_of:
                    source = state_of[name]
                else:
                    if name not in forcing_cols:
                        forcing_cols.append(name)
                    source = -(forcing_cols.index(name) + 1)
                norm = norm_of.setdefault((source, low[j], high[j]), len(norm_of))
                if norm == len(norms):
                    norms.append((source, low[j], high[j]))
                key = (norm, kind, order)
                if key not in factor_of:
                    factor_of[key] = len(factors)
                    factors.append(key)
                row.append(factor_of[key])
            rows.append(row)
        mtxs.append(mtx)
        betas.append(np.ascontiguousarray(b))
        term_factors.append(rows)

    # ---- members ----
    counts = [b.shape[0] for b in betas]
    if len(set(counts)) > 1:
        raise ValueError(f"member e uses selected row e of every model's betas, but the models select {counts} rows: the "
                         f"counts must agree (thin them with draws=)")
    y0 = np.asarray(y0, dtype=np.float64)
    if y0.ndim not in (1, 2) or y0.shape[-1] != K:
        raise ValueError(f"y0 must be [{K}] (one value per state) or [members, {K}]")
    if np.isnan(y0).any():
        raise ValueError("y0 holds NaN")
    E = counts[0]
    if y0.ndim == 2:
        if y0.shape[0] == 0 or (E != 1 and y0.shape[0] != E):
            raise ValueError(f"y0 has {y0.shape[0]} rows but the models select {E} draws: an initial-condition sweep needs one "
                             f"row per member (or one draw, which is shared)")
        E = y0.shape[0]
    cut = bounds_cut(E)
    if ReturnBounds and not 1 <= cut < E:
        raise ValueError(f"bounds (sorted[{cut}], sorted[{E} - {cut}]) need at least 2 members, there "
                         f"{'is' if E == 1 else 'are'} {E}: pass ReturnBounds=False")
    if ReturnBounds and E > MAX_BAND_MEMBERS:
        raise ValueError(f"bounds are formed over at most {MAX_BAND_MEMBERS} members, there are {E}: pass ReturnBounds=False "
                         f"or thin the draws")

    # ---- the box ----
    if bounds is None:
        box = np.stack([range_lo, range_hi], axis=1)
    else:
        box = np.array(bounds, dtype=np.float64)
        if box.shape != (K, 2) or np.isnan(box).any():
            raise ValueError(f"bounds must be [{K}, 2] numbers (true scale): a lower and an upper edge per state")
    for k, name in enumerate(states):
        if not box[k, 0] < box[k, 1]:
            raise ValueError(f"state '{name}': its box is empty (lower {box[k, 0]}, upper {box[k, 1]})" +
                             ("" if bounds is not None else ": the training ranges of the models that read it have no "
                                                            "interval in common"))

    # ---- order: forcing before state (those by state), splines before Bernoulli; slot 0 of the factor values holds 1.0 ----
    norm_order = sorted(range(len(norms)), key=lambda n: (norms[n][0] >= 0, max(norms[n][0], 0), n))
    norm_slot = {n: i for i, n in enumerate(norm_order)}
    n_norm_forcing = sum(1 for n in norms if n[0] < 0)
    fac_order = sorted(range(len(factors)), key=lambda f: (norms[factors[f][0]][0] >= 0, factors[f][1] != SPLINE, f))
    fac_slot = {f: i for i, f in enumerate(fac_order)}
    used = {kind: sorted(o for (kd, o) in tables if kd == kind) for kind in (SPLINE, BERNOULLI)}
    spline_table = np.zeros((len(used[SPLINE]), PIECES, 4))
    for i, order in enumerate(used[SPLINE]):
        spline_table[i] = tables[(SPLINE, order)]
    bern_table = np.zeros((len(used[BERNOULLI]), BERNOULLI_WIDTH))
    for i, order in enumerate(used[BERNOULLI]):
        bern_table[i, :order + 1] = tables[(BERNOULLI, order)]
    fac_norm = np.array([norm_slot[factors[f][0]] for f in fac_order], dtype=np.int32)
    fac_kind = np.array([factors[f][1] for f in fac_order], dtype=np.int32)
    fac_row = np.array([used[factors[f][1]].index(factors[f][2]) for f in fac_order], dtype=np.int32)
    fac_degree = np.array([factors[f][2] if factors[f][1] == BERNOULLI else 3 for f in fac_order], dtype=np.int32)
    n_forcing_factors = int(sum(1 for f in fac_order if norms[factors[f][0]][0] < 0))
    n_coef = int(sum(m.shape[0] + 1 for m in mtxs))
    n_norm_state = len(norms) - n_norm_forcing
    need = 1 + len(factors) + n_norm_state + n_coef
    if lds_per_member and need > LDS_ROWS:
        raise ValueError(f"the system needs {need} values per member in LDS (1 + {len(factors)} factors + {n_norm_state} "
                         f"normalised states + {n_coef} coefficients), a wavefront's {LDS_BUDGET // 1024} KB hold {LDS_ROWS}")

    # ---- terms as 16-byte entries {slot, slot, slot, coefficient}: a fourth factor continues in the next entry ----
    entries, entry_begin, entry_count, constant = [], [], [], []
    coef = np.empty((n_coef, E))
    at = 0
    for k in range(K):
        constant.append(at)
        entry_begin.append(len(entries))
        for i, row in enumerate(term_factors[k]):
            slots = [fac_slot[f] + 1 for f in row]
            while len(slots) > 3:
                entries.append(slots[:3] + [-1])
                slots = slots[3:]
            entries.append(slots + [0] * (3 - len(slots)) + [at + 1 + i])
        entry_count.append(len(entries) - entry_begin[-1])
        coef[at:at + mtxs[k].shape[0] + 1] = np.broadcast_to(betas[k], (E, betas[k].shape[1])).T
        at += mtxs[k].shape[0] + 1
    F = np.zeros((n_steps, len(forcing_cols)))
    for c, name in enumerate(forcing_cols):
        F[:, c] = forcing[name][:n_steps]
    return dict(
        K=K, E=E, n_steps=n_steps, T=T, h=h, states=states, forcing=np.ascontiguousarray(F), cut=cut,
        norm_src=np.array([norms[n][0] for n in norm_order], dtype=np.int32),
        norm_lo=np.array([norms[n][1] for n in norm_order], dtype=np.float64),
        norm_span=np.array([norms[n][2] - norms[n][1] for n in norm_order], dtype=np.float64),
        norm_hi=np.array([norms[n][2] for n in norm_order], dtype=np.float64), forcing_cols=list(forcing_cols),
        n_norm_forcing=n_norm_forcing, n_forcing_factors=n_forcing_factors, fac_norm=fac_norm, fac_kind=fac_kind,
        fac_row=fac_row, fac_degree=fac_degree, spline_table=np.ascontiguousarray(spline_table),
        bern_table=np.ascontiguousarray(bern_table),
        entries=np.ascontiguousarray(np.array(entries, dtype=np.int32).reshape(-1, 4)),
        entry_begin=np.array(entry_begin, dtype=np.int32), entry_count=np.array(entry_count, dtype=np.int32),
        constant=np.array(constant, dtype=np.int32), coef=np.ascontiguousarray(coef),
        y0=np.ascontiguousarray(np.broadcast_to(y0, (E, K)).T), box=np.ascontiguousarray(box),
        want_bounds=bool(ReturnBounds), want_members=keep == 'members', lds_rows=need)


# ---------------------------------------------------------------------------------------------------------
# the statement in numpy, vectorised over members
# ---------------------------------------------------------------------------------------------------------

def _clamped(v):
    acted = (v > 1.0) | (v < 0.0)
    v = np.where(v > 1.0, 1.0, v)
    return np.where(v < 0.0, 0.0, v), acted


def _factor_values(p, fac, xn, first, last):
    for f in range(first, last):
        v = xn[p['fac_norm'][f]]
        if p['fac_kind'][f] == SPLINE:
            fac[f + 1] = spline_value(p['spline_table'][p['fac_row'][f]], v)
        else:
            fac[f + 1] = bernoulli_value(p['bern_table'][p['fac_row'][f], :p['fac_degree'][f] + 1], v)


def _stage(p, fac, xn, at):
    """h * model_k(at) of every state k [K, E] after the slope rule, and per member whether a clamp or the rule acted."""
    K, E = at.shape
    acted = np.zeros(E, dtype=bool)
    for n in range(p['n_norm_forcing'], p['norm_src'].shape[0]):
        xn[n], clamp = _clamped((at[p['norm_src'][n]] - p['norm_lo'][n]) / p['norm_span'][n])
        acted |= clamp
    _factor_values(p, fac, xn, p['n_forcing_factors'], p['fac_norm'].shape[0])
    dy = np.empty((K, E))
    for k in range(K):
        delta, phi = np.zeros(E), np.ones(E)
        for a, b, c, w in p['entries'][p['entry_begin'][k]:p['entry_begin'][k] + p['entry_count'][k]]:
            phi = phi * fac[a]
            phi = phi * fac[b]
            phi = phi * fac[c]
            if w >= 0:
                delta = delta + p['coef'][w] * phi
                phi = np.ones(E)
        s = (delta + p['coef'][p['constant'][k]]) * p['h']
        out = ((at[k] >= p['box'][k, 1]) & (s > 0)) | ((at[k] <= p['box'][k, 0]) & (s < 0))
        dy[k] = np.where(out, 0.0, s)
        acted |= out
    return dy, acted


def _step(p, fac, xn, y, s):
    """Step s of every member: y [K, E] at point s -> (y at point s + 1, per member whether a clamp or the slope rule acted)."""
    E = y.shape[1]
    acted = np.zeros(E, dtype=bool)
    for n in range(p['n_norm_forcing']):
        x = np.full(E, p['forcing'][s, -(p['norm_src'][n] + 1)])
        xn[n], clamp = _clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
        acted |= clamp
    _factor_values(p, fac, xn, 0, p['n_forcing_factors'])
    y, stages_acted = _stages(p, fac, xn, y)
    return y, acted | stages_acted


def _stages(p, fac, xn, y):
    """The four stages of one step of size p['h'] (a number, or one per member) from y [K, E], the forcing factors being in
    ``fac``: -> (y after the step, per member whether a clamp or the slope rule acted)."""
    acted = np.zeros(y.shape[1], dtype=bool)
    dy = total = None
    for st in range(4):
        reach, weight = (1.0 if st == 3 else 0.5), (2.0 if st in (1, 2) else 1.0)
        at = y if st == 0 else y + dy * reach
        dy, stage_acted = _stage(p, fac, xn, at)
        total = dy if st == 0 else total + weight * dy
        acted |= stage_acted
    return y + total / 6, acted


def _run_host(p):
    """-> (members [E, K, P], first_saturation [E] int32)"""
    K, E, S = p['K'], p['E'], p['n_steps']
    y = p['y0'].copy()
    members = np.empty((E, K, S + 1))
    members[:, :, 0] = y.T
    first = np.full(E, -1, dtype=np.int32)
    fac = np.ones((1 + p['fac_norm'].shape[0], E))
    xn = np.zeros((p['norm_src'].shape[0], E))
    for s in range(S):
        y, acted = _step(p, fac, xn, y, s)
        members[:, :, s + 1] = y.T
        first = np.where((first < 0) & acted, np.int32(s), first).astype(np.int32)
    return members, first


def _assemble(p, mean, bounds, members, first):
    res = SimulateResult(t=p['T'], mean=mean, first_saturation=first, saturated_fraction=float(np.mean(first >= 0)),
                         states=list(p['states']))
    if p['want_bounds']:
        res['bounds'] = bounds
    if p['want_members']:
        res['members'] = members
    return res


_SIGNATURE = """
    models      : fitted ``FoKL`` objects, or dicts with betas, mtx, phis, minmax, kernel; model k is d(states[k])/dt.
                  'Cubic Splines' and 'Bernoulli Polynomials' models may be mixed
    states      : the names of the integrated states, one per model
    inputs      : per model the names its input columns read, in the order of its ``mtx`` columns: states or keys of
                  ``forcing``, any order, any subset
    forcing     : {name: [steps]} in true scale; value s serves the four stages of step s
    y0          : [n_states], or [E, n_states] for an initial-condition sweep (true scale)
    t           : (start, stop, h): the points are np.arange(start, stop + h, h)
    draws       : None uses every row of each model's betas, an integer the last rows, an index array those rows
                  (``score``'s convention); member e uses selected row e of every model, so the counts must agree.
                  'mean' runs one member on every model's mean coefficients.  One selected row is shared by the members
                  of an initial-condition sweep
    bounds      : [n_states, 2] the box of the states in true scale; default: per state the intersection of the training
                  ranges (minmax) of the models that read it, unbounded if none does
    ReturnBounds: also the band over the members, ``evaluate``'s order statistics: cut = floor(0.025 E) + 1, lower =
                  sorted[cut], upper = sorted[E - cut] (needs 2 <= E <= 16 384)
    keep        : 'members' also returns every member's trajectory

    Returns a ``SimulateResult`` (a dict with attribute access): t [P], mean [n_states, P], bounds [n_states, P, 2],
    members [E, n_states, P], first_saturation [E] int32 (the first step in which a clamp or the slope rule acted for
    that member, -1: never), saturated_fraction.  Nothing is drawn at random; numpy's stream and the fit are left alone."""


def simulate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True, keep=None,
             device=None):
    """Simulate a system of fitted models over every posterior draw, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep)
    ctx = _device_context(device)
    return _assemble(p, *ctx.simulate_ensemble(p))


def simulate_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                  keep=None):
    """``simulate`` in numpy on this host, vectorised over members: the statement the kernel is tested against (module
    docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep)
    members, first = _run_host(p)
    mean = np.mean(members, axis=0)
    band = None
    if p['want_bounds']:
        srt = np.sort(members, axis=0)
        band = np.stack([srt[p['cut']], srt[p['E'] - p['cut']]], axis=-1)
    return _assemble(p, mean, band, members, first)


simulate.__doc__ += _SIGNATURE
simulate_host.__doc__ += _SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# simulate_adaptive: step doubling on simulate's scheme, on a dyadic grid (module docstring)
# ---------------------------------------------------------------------------------------------------------

MAX_HALVINGS = 12
_KEEP_ADAPTIVE = ('members', 'levels')


def _prepare_adaptive(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                      max_halvings):
    """``_prepare`` and what the error control adds; touches no device."""
    kept = (keep,) if isinstance(keep, str) else keep
    if kept is not None and (not isinstance(kept, (tuple, list)) or not 1 <= len(kept) <= 2 or
                             (len(kept) == 2 and kept[0] == kept[1]) or
                             any(not isinstance(name, str) or name not in _KEEP_ADAPTIVE for name in kept)):
        raise ValueError("keep must be None, 'members', 'levels' or a tuple of the two names")
    kept = tuple(kept or ())
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, 'members' if 'members' in kept else None)
    K = p['K']
    try:
        rtol = float(rtol)
    except (TypeError, ValueError):
        rtol = np.nan
    if not (np.isfinite(rtol) and rtol >= 0):
        raise ValueError(f"rtol must be finite and not negative, got {rtol}")
    if atol is None:
        width = p['box'][:, 1] - p['box'][:, 0]
        for k, name in enumerate(p['states']):
            if not np.isfinite(width[k]):
                raise ValueError(f"state '{name}': its box is unbounded, so the default atol (1e-9 x the box's width) does "
                                 f"not exist: pass atol")
        atol = 1e-9 * width
    else:
        atol = _per('atol', atol, K, 'state')
    if not np.all(np.isfinite(atol) & (atol >= 0)):
        raise ValueError(f"atol must be finite and not negative, got {atol.tolist()}")
    if rtol == 0 and np.any(atol == 0):
        raise ValueError(f"rtol == 0 needs a positive atol for every state (the tolerance of a state would be zero), got atol "
                         f"{atol.tolist()}")
    levels = []
    for value in (min_halvings, max_halvings):
        if isinstance(value, (bool, np.bool_)) or np.ndim(value) != 0 or not isinstance(value, (int, np.integer, float, np.floating)) \
                or int(value) != value:
            raise ValueError(f"min_halvings and max_halvings must be integers with 0 <= min_halvings <= max_halvings <= "
                             f"{MAX_HALVINGS}, got {min_halvings!r} and {max_halvings!r}")
        levels.append(int(value))
    if not 0 <= levels[0] <= levels[1] <= MAX_HALVINGS:
        raise ValueError(f"min_halvings and max_halvings need 0 <= min_halvings <= max_halvings <= {MAX_HALVINGS}, got "
                         f"{levels[0]} and {levels[1]}")
    p.update(rtol=rtol, atol=np.ascontiguousarray(atol, dtype=np.float64), min_halvings=levels[0], max_halvings=levels[1],
             want_levels='levels' in kept)
    return p


def _abs(x):
    return np.where(x < 0, -x, x)


def _run_adaptive_host(p):
    """-> (members [E, K, P], first_saturation, pairs, rejected, max_level, error, first_unresolved, levels [E, steps])"""
    K, E, S = p['K'], p['E'], p['n_steps']
    low, top = p['min_halvings'], p['max_halvings']
    FULL = 1 << top
    rtol, atol, h = p['rtol'], p['atol'], p['h']
    y = p['y0'].copy()
    members = np.empty((E, K, S + 1))
    members[:, :, 0] = y.T
    level = np.full(E, low, dtype=np.int64)
    pairs, rejected = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    max_level, error = np.zeros(E, dtype=np.int32), np.zeros(E)
    first, unresolved = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    levels = np.zeros((E, S), dtype=np.int8)
    fac = np.ones((1 + p['fac_norm'].shape[0], E))
    n_norms = p['norm_src'].shape[0]
    for s in range(S):
        acted = np.zeros(E, dtype=bool)
        xn = np.zeros((n_norms, E))
        for n in range(p['n_norm_forcing']):
            x = np.full(E, p['forcing'][s, -(p['norm_src'][n] + 1)])
            xn[n], clamp = _clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
            acted |= clamp
        _factor_values(p, fac, xn, 0, p['n_forcing_factors'])
        first[(first < 0) & acted] = s
        pos = np.zeros(E, dtype=np.int64)
        while True:
            live = np.flatnonzero(pos < FULL)                         # the members still inside the step: a mask
            if live.size == 0:
                break
            k = level[live]
            g = h * np.ldexp(1.0, -(k + 1))                           # an exact scaling
            q = dict(p, coef=p['coef'][:, live], h=g)
            qfac, qxn, at = np.ascontiguousarray(fac[:, live]), np.zeros((n_norms, live.size)), y[:, live]
            with np.errstate(all='ignore'):
                y1, _ = _stages(dict(q, h=2.0 * g), qfac, qxn, at)
                ya, acted_a = _stages(q, qfac, qxn, at)
                y2, acted_b = _stages(q, qfac, qxn, ya)
                ok, easy = np.ones(live.size, dtype=bool), np.ones(live.size, dtype=bool)
                r = np.zeros(live.size)
                for j in range(K):
                    d = _abs(y2[j] - y1[j])
                    a, b = _abs(at[j]), _abs(y2[j])
                    sc = atol[j] + rtol * np.where(b > a, b, a)
                    ok &= d <= 15.0 * sc
                    easy &= 64.0 * d <= 15.0 * sc
                    ratio = d / (15.0 * sc)
                    r = np.where(ratio > r, ratio, r)
            accept = ok | (k == top)
            took = live[accept]
            ka = k[accept]
            y[:, took] = y2[:, accept]
            pos[took] += FULL >> ka
            pairs[took] += 1
            forced = took[~ok[accept]]
            unresolved[forced[unresolved[forced] < 0]] = s
            hit = took[(acted_a | acted_b)[accept]]
            first[hit[first[hit] < 0]] = s
            ra = r[accept]
            error[took] = np.where(ra > error[took], ra, error[took])
            levels[took, s] = np.maximum(levels[took, s], ka)
            max_level[took] = np.maximum(max_level[took], ka)
            relax = easy[accept] & (ka > low) & (pos[took] % (1 << (top - ka + 1)) == 0)
            level[took[relax]] -= 1
            refused = live[~accept]
            level[refused] += 1
            rejected[refused] += 1
        members[:, :, s + 1] = y.T
    return members, first, pairs, rejected, max_level, error, unresolved, levels


def _assemble_adaptive(p, mean, bounds, members, first, pairs, rejected, max_level, error, unresolved, levels):
    res = _assemble(p, mean, bounds, members, first)
    res.update(pairs=pairs, rejected=rejected, max_level=max_level, error=error, first_unresolved=unresolved,
               unresolved_fraction=float(np.mean(unresolved >= 0)), rtol=p['rtol'], atol=p['atol'])
    if p['want_levels']:
        res['levels'] = levels
    return res


_SIGNATURE_ADAPTIVE = _SIGNATURE.replace("keep        : 'members' also returns every member's trajectory", """\
keep        : None, 'members' (also every member's trajectory), 'levels' (also the deepest level accepted inside each
                  step, [E, steps] int8) or a tuple of the two names
    rtol, atol  : a pair of half steps is accepted where |y2 - y1| / 15 <= atol_j + rtol max(|y_j|, |y2_j|) for every state
                  j; atol is a number or one per state, default per state 1e-9 x (box_hi - box_lo) (a state whose box is
                  unbounded needs an explicit atol)
    min_halvings, max_halvings : the levels k a member may use, 0 <= min <= max <= 12: its substep is h / 2^(k + 1); at
                  k == max_halvings a pair is taken whatever its estimate (``first_unresolved`` records the step)""") + """
    and pairs, rejected [E] int64 (accepted pairs of half steps, rejected trials), max_level [E] int32 (the deepest level
    of an accepted pair), error [E] (the largest accepted |y2 - y1| / (15 sc); <= 1 unless a step was forced),
    first_unresolved [E] int32 (the first step in which the finest level still missed the tolerance, -1: never),
    unresolved_fraction."""


def simulate_adaptive(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                      keep=None, rtol=1e-6, atol=None, min_halvings=0, max_halvings=10, device=None):
    """``simulate`` with an error statement: every member chooses its own substeps inside each output step by step doubling
    on a dyadic grid, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_adaptive(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                          max_halvings)
    ctx = _device_context(device)
    return _assemble_adaptive(p, *ctx.simulate_adaptive(p))


def simulate_adaptive_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                           keep=None, rtol=1e-6, atol=None, min_halvings=0, max_halvings=10):
    """``simulate_adaptive`` in numpy on this host, vectorised over members with masks: the statement the kernel is tested
    against (module docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare_adaptive(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                          max_halvings)
    members, *record = _run_adaptive_host(p)
    mean = np.mean(members, axis=0)
    band = None
    if p['want_bounds']:
        srt = np.sort(members, axis=0)
        band = np.stack([srt[p['cut']], srt[p['E'] - p['cut']]], axis=-1)
    return _assemble_adaptive(p, mean, band, members, *record)


simulate_adaptive.__doc__ += _SIGNATURE_ADAPTIVE
simulate_adaptive_host.__doc__ += _SIGNATURE_ADAPTIVE


# ---------------------------------------------------------------------------------------------------------
# simulate_stiff: Rodas3 under simulate_adaptive's dyadic controller (module docstring)
# ---------------------------------------------------------------------------------------------------------

def stiff_lds_rows(n_factors, n_norm_state, n_coef):
    """Values per member the stiff kernel holds in LDS: ``simulate``'s and one set of tangent rows."""
    return 2 * (1 + n_factors + n_norm_state) + n_coef


def _prepare_stiff(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                   max_halvings):
    """``_prepare_adaptive`` and the LDS need of the tangent rows; touches no device."""
    p = _prepare_adaptive(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                          max_halvings)
    n_factors, n_norm_state, n_coef = p['fac_norm'].shape[0], p['norm_src'].shape[0] - p['n_norm_forcing'], p['coef'].shape[0]
    need = stiff_lds_rows(n_factors, n_norm_state, n_coef)
    if need > LDS_ROWS:
        raise ValueError(f"the system needs {need} values per member in LDS (2 x (1 + {n_factors} factors + {n_norm_state} "
                         f"normalised states) + {n_coef} coefficients: simulate's and one set of tangent rows), a wavefront's "
                         f"{LDS_BUDGET // 1024} KB hold {LDS_ROWS}")
    p['lds_rows'] = need
    return p


def _stage_dual(p, fac, xn, at):
    """F(at) [K, M] (the stage with a step of 1), J [K, K, M] with J[r, d] = d F_r / d y_d, and per member whether a clamp or
    the slope rule acted.  Direction d is axis 1 of every tangent; each is formed as if it were alone."""
    K, M = at.shape
    nF, nN, nNF, nFF = p['fac_norm'].shape[0], p['norm_src'].shape[0], p['n_norm_forcing'], p['n_forcing_factors']
    cf = p['coef']
    acted = np.zeros(M, dtype=bool)
    txn, tfac = np.zeros((nN, K, M)), np.zeros((1 + nF, K, M))
    unit = np.eye(K)
    for n in range(nNF, nN):
        j = p['norm_src'][n]
        xn[n], clamp = _clamped((at[j] - p['norm_lo'][n]) / p['norm_span'][n])
        acted |= clamp
        txn[n] = np.where(clamp, 0.0, np.broadcast_to(unit[j][:, np.newaxis], (K, M)) / p['norm_span'][n])
    for f in range(nFF, nF):
        n = p['fac_norm'][f]
        fac[f + 1], slope = _factor_dual(p, f, xn[n])
        tfac[f + 1] = slope * txn[n]
    F, J = np.empty((K, M)), np.empty((K, K, M))
    zero = np.zeros((K, M))
    for k in range(K):
        delta, phi = np.zeros(M), np.ones(M)
        tdelta, tphi = zero, zero
        for a, b, c, w in p['entries'][p['entry_begin'][k]:p['entry_begin'][k] + p['entry_count'][k]]:
            for slot in (a, b, c):
                tphi = tphi * fac[slot] + phi * tfac[slot]
                phi = phi * fac[slot]
            if w >= 0:
                delta = delta + cf[w] * phi
                tdelta = tdelta + cf[w] * tphi
                phi, tphi = np.ones(M), zero
        s = delta + cf[p['constant'][k]]
        out = ((at[k] >= p['box'][k, 1]) & (s > 0)) | ((at[k] <= p['box'][k, 0]) & (s < 0))
        F[k] = np.where(out, 0.0, s)
        J[k] = np.where(out, 0.0, tdelta)
        acted |= out
    return F, J, acted


def stiff_lu(W):
    """LU with partial pivoting of W [K, K, M], one matrix per member, in the statement's order (module docstring) ->
    (LU [K, K, M]: U on and above the diagonal, the multipliers below it; rows [K, M]: the row exchanged with row c in
    column c; exchanges [M])."""
    W = np.array(W, dtype=np.float64)
    K, M = W.shape[0], W.shape[2]
    rows, exchanges = np.empty((K, M), dtype=np.int64), np.zeros(M, dtype=np.int64)
    for c in range(K):
        best, row = _abs(W[c, c]), np.full(M, c, dtype=np.int64)
        for r in range(c + 1, K):
            a = _abs(W[r, c])
            take = a > best
            best, row = np.where(take, a, best), np.where(take, r, row)
        rows[c] = row
        exchanges += row != c
        for r in range(c + 1, K):
            here = row == r
            upper = W[c, c:].copy()
            W[c, c:] = np.where(here, W[r, c:], upper)
            W[r, c:] = np.where(here, upper, W[r, c:])
        for r in range(c + 1, K):
            l = W[r, c] / W[c, c]
            W[r, c] = l
            for j in range(c + 1, K):
                W[r, j] = W[r, j] - l * W[c, j]
    return W, rows, exchanges


def stiff_solve(LU, rows, b):
    """``stiff_lu``'s factors applied to b [K, M] -> W^-1 b, in the statement's order."""
    b = np.array(b, dtype=np.float64)
    K = b.shape[0]
    for c in range(K):
        for r in range(c + 1, K):
            here = rows[c] == r
            upper = b[c].copy()
            b[c] = np.where(here, b[r], upper)
            b[r] = np.where(here, upper, b[r])
        for r in range(c + 1, K):
            b[r] = b[r] - LU[r, c] * b[c]
    for c in range(K - 1, -1, -1):
        b[c] = b[c] / LU[c, c]
        for r in range(c):
            b[r] = b[r] - LU[r, c] * b[c]
    return b


def _stiff_trial(q, qfac, qxn, y, g):
    """One Rodas3 trial of size g [M] from y [K, M] with the forcing factors in ``qfac`` -> (y_new, K4, exchanges, acted,
    W, LU, rows, F0, K1)."""
    K = y.shape[0]
    c2, c4, ig, c83 = 2.0 / g, 4.0 / g, 1.0 / g, 8.0 / 3.0
    F0, J, acted = _stage_dual(q, qfac, qxn, y)
    W = -J
    for r in range(K):
        W[r, r] = c2 - J[r, r]
    LU, rows, exchanges = stiff_lu(W)
    K1 = stiff_solve(LU, rows, F0)
    K2 = stiff_solve(LU, rows, F0 + c4 * K1)
    y3 = y + 2.0 * K1
    F3, acted3 = _stage(q, qfac, qxn, y3)
    K3 = stiff_solve(LU, rows, F3 + (K1 - K2) * ig)
    y4 = y3 + K3
    F4, acted4 = _stage(q, qfac, qxn, y4)
    K4 = stiff_solve(LU, rows, F4 + ((K1 - K2) - c83 * K3) * ig)
    return y4 + K4, K4, exchanges, acted | acted3 | acted4, W, LU, rows, F0, K1


def _run_stiff_host(p, trial_hook=None):
    """-> (members [E, K, P], first_saturation, steps, rejected, swaps, max_level, error, first_unresolved, levels [E, steps]).
    ``trial_hook(s, live, W, LU, rows, F0, K1)`` sees every trial (tests)."""
    K, E, S = p['K'], p['E'], p['n_steps']
    low, top = p['min_halvings'], p['max_halvings']
    FULL = 1 << top
    rtol, atol, h = p['rtol'], p['atol'], p['h']
    y = p['y0'].copy()
    members = np.empty((E, K, S + 1))
    members[:, :, 0] = y.T
    level = np.full(E, low, dtype=np.int64)
    steps, rejected, swaps = (np.zeros(E, dtype=np.int64) for _ in range(3))
    max_level, error = np.zeros(E, dtype=np.int32), np.zeros(E)
    first, unresolved = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    levels = np.zeros((E, S), dtype=np.int8)
    fac = np.ones((1 + p['fac_norm'].shape[0], E))
    n_norms = p['norm_src'].shape[0]
    for s in range(S):
        acted = np.zeros(E, dtype=bool)
        xn = np.zeros((n_norms, E))
        for n in range(p['n_norm_forcing']):
            x = np.full(E, p['forcing'][s, -(p['norm_src'][n] + 1)])
            xn[n], clamp = _clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
            acted |= clamp
        _factor_values(p, fac, xn, 0, p['n_forcing_factors'])
        first[(first < 0) & acted] = s
        pos = np.zeros(E, dtype=np.int64)
        while True:
            live = np.flatnonzero(pos < FULL)                         # the members still inside the step: a mask
            if live.size == 0:
                break
            k = level[live]
            g = h * np.ldexp(1.0, -k)                                 # an exact scaling
            q = dict(p, coef=p['coef'][:, live], h=1.0)
            qfac, qxn, at = np.ascontiguousarray(fac[:, live]), np.zeros((n_norms, live.size)), y[:, live]
            with np.errstate(all='ignore'):
                y_new, est, exchanges, trial_acted, *seen = _stiff_trial(q, qfac, qxn, at, g)
                ok, easy = np.ones(live.size, dtype=bool), np.ones(live.size, dtype=bool)
                r = np.zeros(live.size)
                for j in range(K):
                    d = _abs(est[j])
                    a, b = _abs(at[j]), _abs(y_new[j])
                    sc = atol[j] + rtol * np.where(b > a, b, a)
                    ok &= d <= sc
                    easy &= 16.0 * d <= sc
                    ratio = d / sc
                    r = np.where(ratio > r, ratio, r)
            if trial_hook is not None:
                trial_hook(s, live, *seen)
            accept = ok | (k == top)
            took = live[accept]
            ka = k[accept]
            y[:, took] = y_new[:, accept]
            pos[took] += FULL >> ka
            steps[took] += 1
            swaps[took] += exchanges[accept]
            forced = took[~ok[accept]]
            unresolved[forced[unresolved[forced] < 0]] = s
            hit = took[trial_acted[accept]]
            first[hit[first[hit] < 0]] = s
            ra = r[accept]
            error[took] = np.where(ra > error[took], ra, error[took])
            levels[took, s] = np.maximum(levels[took, s], ka)
            max_level[took] = np.maximum(max_level[took], ka)
            relax = easy[accept] & (ka > low) & (pos[took] % (1 << (top - ka + 1)) == 0)
            level[took[relax]] -= 1
            refused = live[~accept]
            level[refused] += 1
            rejected[refused] += 1
        members[:, :, s + 1] = y.T
    return members, first, steps, rejected, swaps, max_level, error, unresolved, levels


def _assemble_stiff(p, mean, bounds, members, first, steps, rejected, swaps, max_level, error, unresolved, levels):
    res = _assemble(p, mean, bounds, members, first)
    res.update(steps=steps, rejected=rejected, swaps=swaps, max_level=max_level, error=error, first_unresolved=unresolved,
               unresolved_fraction=float(np.mean(unresolved >= 0)), rtol=p['rtol'], atol=p['atol'])
    if p['want_levels']:
        res['levels'] = levels
    return res


_SIGNATURE_STIFF = _SIGNATURE.replace("keep        : 'members' also returns every member's trajectory", """\
keep        : None, 'members' (also every member's trajectory), 'levels' (also the deepest level accepted inside each
                  step, [E, steps] int8) or a tuple of the two names
    rtol, atol  : a step is accepted where the embedded estimate |K4_j| <= atol_j + rtol max(|y_j|, |y_new_j|) for every state
                  j; atol is a number or one per state, default per state 1e-9 x (box_hi - box_lo) (a state whose box is
                  unbounded needs an explicit atol)
    min_halvings, max_halvings : the levels k a member may use, 0 <= min <= max <= 12: its step is h / 2^k; at
                  k == max_halvings a step is taken whatever its estimate (``first_unresolved`` records the output step)""") + """
    and steps, rejected, swaps [E] int64 (accepted steps, rejected trials, row exchanges of the accepted steps' factorisations),
    max_level [E] int32 (the deepest level of an accepted step), error [E] (the largest accepted |K4| / sc; <= 1 unless a
    step was forced), first_unresolved [E] int32 (the first output step in which the finest level still missed the tolerance,
    -1: never), unresolved_fraction."""


def simulate_stiff(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                   keep=None, rtol=1e-4, atol=None, min_halvings=0, max_halvings=10, device=None):
    """``simulate_adaptive`` for stiff members: the linearly implicit Rodas3 step (order 3, L-stable) under the same per-member
    dyadic step control, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_stiff(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                       max_halvings)
    ctx = _device_context(device)
    return _assemble_stiff(p, *ctx.simulate_stiff(p))


def simulate_stiff_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, ReturnBounds=True,
                        keep=None, rtol=1e-4, atol=None, min_halvings=0, max_halvings=10, trial_hook=None):
    """``simulate_stiff`` in numpy on this host, vectorised over members with masks: the statement the kernel is tested
    against (module docstring), not a fallback.  Same arguments, same result fields.  ``trial_hook(s, live, W, LU, rows,
    F0, K1)`` is called with every trial's matrix, its factors, F(y) and the first stage, for the members ``live`` of output step s."""
    p = _prepare_stiff(models, states, inputs, forcing, y0, t, draws, bounds, ReturnBounds, keep, rtol, atol, min_halvings,
                       max_halvings)
    members, *record = _run_stiff_host(p, trial_hook)
    mean = np.mean(members, axis=0)
    band = None
    if p['want_bounds']:
        srt = np.sort(members, axis=0)
        band = np.stack([srt[p['cut']], srt[p['E'] - p['cut']]], axis=-1)
    return _assemble_stiff(p, mean, band, members, *record)


simulate_stiff.__doc__ += _SIGNATURE_STIFF
simulate_stiff_host.__doc__ += _SIGNATURE_STIFF


# ---------------------------------------------------------------------------------------------------------
# steady_states: a damped Newton iteration on simulate_stiff's F and J per (operating point, draw, start) (module docstring)
# ---------------------------------------------------------------------------------------------------------

STEADY_MAX_ITER = 200
STEADY_MAX_HALVINGS = 30
_HALTON_BASES = (2, 3, 5, 7, 11, 13, 17, 19)


class SteadyResult(SimulateResult):
    """``steady_states``'s result: a dict whose entries are also attributes."""


def _radical_inverse(i, base):
    r, f = 0.0, 1.0
    while i > 0:
        f = f / base
        r = r + f * (i % base)
        i //= base
    return r


def steady_starts(S, box):
    """The S starts of an integer ``starts`` in the box [K, 2]: its centre, then Halton points (module docstring) -> [S, K]."""
    lo, width = box[:, 0], box[:, 1] - box[:, 0]
    out = np.empty((S, box.shape[0]))
    out[0] = lo + width * 0.5
    for i in range(1, S):
        out[i] = lo + np.array([_radical_inverse(i, _HALTON_BASES[j]) for j in range(box.shape[0])]) * width
    return out


def _whole(name, value, low, high):
    if isinstance(value, (bool, np.bool_)) or np.ndim(value) != 0 or not isinstance(value, (int, np.integer, float, np.floating)) \
            or int(value) != value or not low <= int(value) <= high:
        raise ValueError(f"{name} must be an integer in {low}..{high}, got {value!r}")
    return int(value)


def _prepare_steady(models, states, inputs, at, draws, bounds, starts, ftol, time_scale, max_iter, max_halvings, merge_tol, keep):
    """``_prepare`` with the operating points as forcing rows, and what the iteration adds; touches no device."""
    if keep not in (None, 'jacobian'):
        raise ValueError("keep must be None or 'jacobian'")
    names = [str(name) for name in states]
    at = {str(name): np.asarray(values, dtype=np.float64) for name, values in dict(at or {}).items()}
    both = [name for name in at if name in names]
    if both:
        raise ValueError(f"at: {both} are states: a state is solved for, not given")
    read = []
    for columns in inputs:
        read += [str(name) for name in columns if str(name) not in names and str(name) not in read]
    missing = [name for name in read if name not in at]
    if missing:
        raise ValueError(f"at: the input columns {missing} are no states and at gives no value for them (at holds {list(at)})")
    lengths = {}
    for name, values in at.items():
        if values.ndim > 1 or (values.ndim == 1 and values.shape[0] == 0):
            raise ValueError(f"at['{name}'] must be a number or [Q] values, Q >= 1")
        if values.ndim == 1:
            lengths[name] = values.shape[0]
    if len(set(lengths.values())) > 1:
        raise ValueError(f"at: the arrays have unequal lengths {lengths}: every array holds one value per operating point")
    Q = next(iter(lengths.values()), 1)
    forcing = {name: np.array(np.broadcast_to(values, (Q,))) for name, values in at.items()}
    for name, values in forcing.items():
        if not np.isfinite(values).all():
            raise ValueError(f"at['{name}'] must hold finite numbers")
    max_iter = _whole('max_iter', max_iter, 1, STEADY_MAX_ITER)
    max_halvings = _whole('max_halvings', max_halvings, 0, STEADY_MAX_HALVINGS)
    try:
        time_scale, merge_tol = float(time_scale), float(merge_tol)
    except (TypeError, ValueError):
        time_scale, merge_tol = np.nan, np.nan
    if not (np.isfinite(time_scale) and time_scale > 0):
        raise ValueError(f"time_scale must be positive and finite, got {time_scale}")
    if not (np.isfinite(merge_tol) and merge_tol >= 0):
        raise ValueError(f"merge_tol must be finite and not negative, got {merge_tol}")

    p = _prepare(models, names, inputs, forcing, np.zeros(len(names)), (0.0, float(Q), 1.0), draws, bounds, False, None)
    K, box = p['K'], p['box']
    n_factors, n_norm_state, n_coef = p['fac_norm'].shape[0], p['norm_src'].shape[0] - p['n_norm_forcing'], p['coef'].shape[0]
    need = stiff_lds_rows(n_factors, n_norm_state, n_coef)
    if need > LDS_ROWS:
        raise ValueError(f"the system needs {need} values per member in LDS (2 x (1 + {n_factors} factors + {n_norm_state} "
                         f"normalised states) + {n_coef} coefficients: simulate's and one set of tangent rows), a wavefront's "
                         f"{LDS_BUDGET // 1024} KB hold {LDS_ROWS}")
    width = box[:, 1] - box[:, 0]
    unbounded = [name for k, name in enumerate(names) if not np.isfinite(width[k])]
    if isinstance(starts, (bool, np.bool_)) or (np.ndim(starts) == 0 and not isinstance(starts, (int, np.integer))):
        raise ValueError(f"starts must be an integer S >= 1 or an array [S, {K}], got {starts!r}")
    if np.ndim(starts) == 0:
        if int(starts) < 1:
            raise ValueError(f"starts must be an integer S >= 1 or an array [S, {K}], got {starts!r}")
        if unbounded:
            raise ValueError(f"states {unbounded}: the box is unbounded, so the centre and the Halton points of starts={starts} "
                             f"do not exist: pass starts as an array [S, {K}] (or bounds)")
        starts = steady_starts(int(starts), box)
    else:
        starts = np.array(starts, dtype=np.float64)
        if starts.ndim != 2 or starts.shape[0] == 0 or starts.shape[1] != K:
            raise ValueError(f"starts as an array must be [S, {K}] (true scale), S >= 1, got shape {starts.shape}")
        if np.isnan(starts).any():
            raise ValueError("starts holds NaN")
        outside = (starts < box[:, 0]) | (starts > box[:, 1])
        if outside.any():
            s, k = np.argwhere(outside)[0]
            raise ValueError(f"starts[{s}]: state '{names[k]}' = {starts[s, k]} lies outside its box [{box[k, 0]}, {box[k, 1]}]")
    if ftol is None:
        if unbounded:
            raise ValueError(f"states {unbounded}: the box is unbounded, so the default ftol (1e-9 x the box's width / time_scale) "
                             f"does not exist: pass ftol")
        ftol = 1e-9 * width / time_scale
    else:
        ftol = _per('ftol', ftol, K, 'state')
    if not np.all(np.isfinite(ftol) & (ftol > 0)):
        raise ValueError(f"ftol must be positive and finite for every state, got {np.asarray(ftol).tolist()}")
    p.update(Q=Q, S=starts.shape[0], starts=np.ascontiguousarray(starts), ftol=np.ascontiguousarray(ftol, dtype=np.float64),
             max_iter=max_iter, max_halvings=max_halvings, merge_tol=merge_tol, want_jacobian=keep == 'jacobian', lds_rows=need,
             at={name: forcing[name] for name in forcing})
    return p


def _steady_ratio(F, ftol):
    r = np.zeros(F.shape[1])
    for j in range(F.shape[0]):
        q = _abs(F[j]) / ftol[j]
        r = np.where((q > r) | (q != q), q, r)
    return r


def _run_steady_host(p):
    """-> (y [Q, M, K], residual [Q, M], iterations [Q, M] int32, status [Q, M] int8, halvings [Q, M] int32, on_wall [Q, M, K]
    bool, jacobian [Q, M, K, K]) with M = E S, member e S + s of a point being draw e from start s."""
    K, E, S, Q = p['K'], p['E'], p['S'], p['Q']
    top, limit, ftol, box = p['max_halvings'], p['max_iter'], p['ftol'], p['box']
    N = Q * E * S
    point, draw, start = np.repeat(np.arange(Q), E * S), np.tile(np.repeat(np.arange(E), S), Q), np.tile(np.arange(S), Q * E)
    coef = p['coef'][:, draw]
    y = np.ascontiguousarray(p['starts'].T[:, start])
    n_norms = p['norm_src'].shape[0]
    fac, xn = np.ones((1 + p['fac_norm'].shape[0], N)), np.zeros((n_norms, N))
    for n in range(p['n_norm_forcing']):
        xn[n], _ = _clamped((p['forcing'][point, -(p['norm_src'][n] + 1)] - p['norm_lo'][n]) / p['norm_span'][n])
    _factor_values(p, fac, xn, 0, p['n_forcing_factors'])
    status = np.full(N, -1, dtype=np.int8)
    iterations, halvings = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    residual, jacobian, on_wall = np.full(N, np.nan), np.full((N, K, K), np.nan), np.zeros((N, K), dtype=bool)
    with np.errstate(all='ignore'):
        for it in range(limit + 1):
            live = np.flatnonzero(status < 0)                         # the members still iterating: a mask
            if live.size == 0:
                break
            q = dict(p, coef=coef[:, live], h=1.0)
            qfac, at = np.ascontiguousarray(fac[:, live]), y[:, live]
            F, J, _ = _stage_dual(q, qfac, np.zeros((n_norms, live.size)), at)
            r = _steady_ratio(F, ftol)
            held = (F == 0) & ~np.any(J != 0, axis=1)
            residual[live], jacobian[live], on_wall[live] = r, J.transpose(2, 0, 1), held.T
            ended = np.where(~(r < np.inf), 3, np.where(r <= 1, 0, 1 if it == limit else -1)).astype(np.int8)
            status[live] = ended
            go = ended < 0
            if not go.any():
                continue
            live, F, J, r, held, at, qfac = live[go], F[:, go], J[:, :, go], r[go], held[:, go], at[:, go], qfac[:, go]
            W = -J
            for k in range(K):
                W[k, k] = np.where(held[k], 1.0, W[k, k])
            LU, rows, _ = stiff_lu(W)
            delta = np.where(held, 0.0, stiff_solve(LU, rows, F))
            found = np.zeros(live.size, dtype=bool)
            for b in range(top + 1):
                todo = np.flatnonzero(~found)
                if todo.size == 0:
                    break
                yt = at[:, todo] + delta[:, todo] * np.ldexp(1.0, -b)
                yt = np.where(yt < box[:, :1], box[:, :1], yt)
                yt = np.where(yt > box[:, 1:], box[:, 1:], yt)
                Ft, _ = _stage(dict(p, coef=coef[:, live[todo]], h=1.0), np.ascontiguousarray(qfac[:, todo]),
                               np.zeros((n_norms, todo.size)), yt)
                ok = _steady_ratio(Ft, ftol) < r[todo]
                took = todo[ok]
                y[:, live[took]] = yt[:, ok]
                halvings[live[took]] += b
                found[took] = True
            status[live[~found]] = 2
            halvings[live[~found]] += top + 1
            iterations[live[found]] += 1
    M = E * S
    return (np.ascontiguousarray(y.T).reshape(Q, M, K), residual.reshape(Q, M), iterations.reshape(Q, M), status.reshape(Q, M),
            halvings.reshape(Q, M), on_wall.reshape(Q, M, K), jacobian.reshape(Q, M, K, K))


def _steady_roots(y, converged, stable, tol):
    """The distinct roots among the converged members of every (point, draw): y [N, S, K], converged and stable [N, S] ->
    (roots [N, S, K], root_stable [N, S], n_roots [N]; the first n_roots[i] entries of row i count).  In lexicographic order a
    member joins the first root it is within ``tol`` of in every state, or founds one; all N rows at once."""
    N, S, K = y.shape
    order = np.lexsort(tuple(y[..., k] for k in range(K - 1, -1, -1)) + (~converged,), axis=-1)
    rows = np.arange(N)
    roots, flags, count = np.full((N, S, K), np.nan), np.zeros((N, S), dtype=bool), np.zeros(N, dtype=np.int64)
    for i in range(S):
        at = order[:, i]
        point, joined = y[rows, at], ~converged[rows, at]
        for r in range(int(count.max(initial=0))):
            with np.errstate(invalid='ignore'):
                joined |= (r < count) & np.all(np.abs(point - roots[:, r]) <= tol, axis=1)
        new = np.flatnonzero(~joined)
        roots[new, count[new]], flags[new, count[new]] = point[new], stable[new, at[new]]
        count[new] += 1
    return roots, flags, count


def _assemble_steady(p, y, residual, iterations, status, halvings, on_wall, jacobian):
    """The result from the per-member fields, the same numpy after the device and the host statement."""
    K, E, S, Q = p['K'], p['E'], p['S'], p['Q']
    shape = (Q, E, S)
    y, residual, iterations = y.reshape(shape + (K,)), residual.reshape(shape), iterations.reshape(shape).astype(np.int32)
    status, halvings = status.reshape(shape).astype(np.int8), halvings.reshape(shape).astype(np.int32)
    on_wall, jacobian = on_wall.reshape(shape + (K,)).astype(bool), jacobian.reshape(shape + (K, K))
    converged = status == 0
    eig = np.full(shape + (K,), np.nan + 0j, dtype=np.complex128)
    flat_wall, flat_jac, flat_eig = on_wall.reshape(-1, K), jacobian.reshape(-1, K, K), eig.reshape(-1, K)
    patterns, which = np.unique(flat_wall, axis=0, return_inverse=True)
    which = which.reshape(-1)
    negative = np.ones(flat_wall.shape[0], dtype=bool)                # no free state: nothing can grow
    for i, held in enumerate(patterns):                               # one batched call per set of held states
        free, rows = np.flatnonzero(~held), np.flatnonzero(which == i)
        if free.size == 0:
            continue
        blocks = flat_jac[rows][:, free][:, :, free]
        finite = np.isfinite(blocks).all(axis=(1, 2))
        values = np.full((rows.size, free.size), np.nan + 0j, dtype=np.complex128)
        if finite.any():
            values[finite] = np.linalg.eigvals(blocks[finite])
        flat_eig[np.ix_(rows, free)] = values
        negative[rows] = np.all(values.real < 0, axis=1)
    stable = converged & negative.reshape(shape)
    width = p['box'][:, 1] - p['box'][:, 0]
    tol = p['merge_tol'] * np.where(np.isfinite(width), width, 1.0)
    found, flags, count = _steady_roots(y.reshape(Q * E, S, K), converged.reshape(Q * E, S), stable.reshape(Q * E, S), tol)
    roots = [[found[q * E + e, :count[q * E + e]] for e in range(E)] for q in range(Q)]
    root_stable = [[flags[q * E + e, :count[q * E + e]] for e in range(E)] for q in range(Q)]
    n_roots = count.reshape(Q, E)
    n_stable = np.sum(flags, axis=1).reshape(Q, E)
    most = int(n_roots.max())
    multiplicity = np.stack([np.mean(n_roots == k, axis=1) for k in range(most + 1)], axis=1)
    unique_mean, unique_bounds = np.full((Q, K), np.nan), np.full((Q, K, 2), np.nan)
    for q in range(Q):
        single = [roots[q][e][0] for e in range(E) if n_roots[q, e] == 1]
        if len(single) >= 2:
            srt, cut = np.sort(np.array(single), axis=0), bounds_cut(len(single))
            unique_mean[q] = np.mean(np.array(single), axis=0)
            unique_bounds[q] = np.stack([srt[cut], srt[len(single) - cut]], axis=-1)
    res = SteadyResult(states=list(p['states']), at=p['at'], starts=p['starts'], ftol=p['ftol'], y=y, residual=residual,
                       iterations=iterations, status=status, halvings=halvings, on_wall=on_wall, stable=stable, roots=roots,
                       root_stable=root_stable, n_roots=n_roots, n_stable=n_stable, multiplicity=multiplicity,
                       unique_fraction=np.mean(n_roots == 1, axis=1), unique_mean=unique_mean, unique_bounds=unique_bounds)
    if p['want_jacobian']:
        res.update(jacobian=jacobian, eig=eig)
    return res


_STEADY_SIGNATURE = """
    models, states, inputs, draws, bounds : as ``simulate``'s
    at          : {name: a number or [Q] values} in true scale, one entry per input column that is not a state; numbers are
                  shared by the Q >= 1 operating points
    starts      : an integer S (the centre of the box and S - 1 Halton points inside it; needs a bounded box) or [S, n_states]
                  in true scale inside the closed box; every (point, draw) iterates from every start
    ftol        : a number or one per state, default 1e-9 x (box_hi - box_lo) / time_scale: a member has converged where
                  max_j |F_j| / ftol_j <= 1
    time_scale  : the time in which a state crosses its box at a slope worth resolving; it only scales the default ftol
    max_iter    : 1..200 Newton iterations per member;  max_halvings : 0..30 halvings of a step in its line search
    merge_tol   : converged members of one (point, draw) within merge_tol x (box_hi - box_lo) in every state are one root
                  (merge_tol itself for a state whose box is unbounded)
    keep        : 'jacobian' also returns ``jacobian`` and ``eig``

    Returns a ``SteadyResult`` (a dict with attribute access).  Per member (point q, draw e, start s): y [Q, E, S, n], residual
    [Q, E, S], iterations int32, status int8 (0 converged, 1 iteration limit, 2 stalled, 3 not finite), halvings int32,
    on_wall [Q, E, S, n] bool (the state was held at the end), stable [Q, E, S] (converged and every eigenvalue of the
    Jacobian's free sub-block has a negative real part), with keep='jacobian' jacobian [Q, E, S, n, n] and eig [Q, E, S, n]
    complex (NaN at held states).  Per (point, draw): roots[q][e] [R, n] sorted lexicographically, root_stable[q][e] [R], n_roots
    and n_stable [Q, E].  Over the draws: multiplicity [Q, Rmax + 1] (the share of draws with k distinct roots),
    unique_fraction [Q], unique_mean [Q, n] and unique_bounds [Q, n, 2] over the draws with exactly one root (``evaluate``'s order
    statistics; NaN with fewer than two such draws).  It finds the roots its starts lead to and does not prove that there are no
    others; a root on a wall is a rest point of the clamped system, not of the models; Newton does not prefer stable roots.
    Nothing is drawn at random."""


def steady_states(models, states, inputs, at=None, draws=None, bounds=None, starts=9, ftol=None, time_scale=1.0, max_iter=50,
                  max_halvings=8, merge_tol=1e-6, keep=None, device=None):
    """The rest points of a system of fitted models and their stability, per operating point, posterior draw and start, on the
    device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_steady(models, states, inputs, at, draws, bounds, starts, ftol, time_scale, max_iter, max_halvings, merge_tol, keep)
    ctx = _device_context(device)
    return _assemble_steady(p, *ctx.steady_states(p))


def steady_states_host(models, states, inputs, at=None, draws=None, bounds=None, starts=9, ftol=None, time_scale=1.0, max_iter=50,
                       max_halvings=8, merge_tol=1e-6, keep=None):
    """``steady_states`` in numpy on this host, vectorised over members with masks: the statement the kernel is tested against
    (module docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare_steady(models, states, inputs, at, draws, bounds, starts, ftol, time_scale, max_iter, max_halvings, merge_tol, keep)
    return _assemble_steady(p, *_run_steady_host(p))


steady_states.__doc__ += _STEADY_SIGNATURE
steady_states_host.__doc__ += _STEADY_SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# assimilate: a bootstrap particle filter per posterior draw (module docstring)
# ---------------------------------------------------------------------------------------------------------

PARTICLES = _capi.ASSIMILATE_PARTICLES
LW_FLOOR = -745.0                         # below it exp() of the best particle's log weight is no positive double
_LANES = np.arange(PARTICLES)


def lane_sum(v):
    """The sum over the last axis (64 lanes) as the xor butterfly forms it: every lane's value, all the same bits."""
    v = np.array(v, dtype=np.float64)
    for offset in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ offset]
    return v[..., 0]


def lane_max(v):
    """The maximum over the last axis (64 lanes) by the same butterfly; fmax passes over a NaN."""
    v = np.array(v, dtype=np.float64)
    for offset in (32, 16, 8, 4, 2, 1):
        v = np.fmax(v, v[..., _LANES ^ offset])
    return v[..., 0]


def lane_scan(v):
    """The inclusive prefix sum over the last axis (64 lanes) as the Hillis-Steele scan forms it."""
    v = np.array(v, dtype=np.float64)
    for offset in (1, 2, 4, 8, 16, 32):
        v = np.concatenate([v[..., :offset], v[..., offset:] + v[..., :-offset]], axis=-1)
    return v


def systematic_ancestors(W, u):
    """W [..., 64] weights, u [...] in [0, 1) -> the ancestor of every particle [..., 64] (module docstring)."""
    c = lane_scan(W)
    target = (_LANES + np.asarray(u, dtype=np.float64)[..., np.newaxis]) / float(PARTICLES) * c[..., PARTICLES - 1:]
    count = np.sum(c[..., np.newaxis, :] <= target[..., :, np.newaxis], axis=-1)
    return np.minimum(count, PARTICLES - 1)


def _draw_ids(n_rows, draws, E):
    if draws is None:
        ids = np.arange(n_rows)
    elif isinstance(draws, str):
        ids = np.zeros(1, dtype=np.int64)
    elif np.ndim(draws) == 0:
        ids = np.arange(n_rows - int(draws), n_rows)
    else:
        ids = np.asarray(draws) % n_rows
    if ids.shape[0] != E:                                             # one draw shared by an initial-condition sweep
        ids = np.arange(E)
    return ids.astype(np.uint32)


def _per(name, values, count, what):
    try:
        out = np.array(np.broadcast_to(np.asarray(values, dtype=np.float64), (count,)))
    except ValueError:
        raise ValueError(f"{name} needs one value per {what} ({count}), got shape {np.shape(values)}") from None
    return out


def _prepare_observations(states, P, observe, data, obs_points, every, obs_sd):
    """The checks of ``observe``, ``data``, ``obs_points`` / ``every`` and ``obs_sd`` that ``assimilate`` and ``calibrate``
    share -> (names, points, data, obs_sd)."""
    names = [str(name) for name in (observe if observe is not None else [])]
    if not names:
        raise ValueError("observe must name at least one measured state")
    for name in names:
        if name not in states:
            raise ValueError(f"observe: '{name}' is not a state ({states})")
    if len(set(names)) != len(names):
        raise ValueError(f"observe names a state twice: {names}")
    if (obs_points is None) == (every is None):
        raise ValueError("give either obs_points (indices into t) or every (points k, 2k, ...): exactly one of the two")
    if every is not None:
        if np.ndim(every) != 0 or int(every) != every or int(every) < 1:
            raise ValueError("every must be a positive integer")
        points = np.arange(int(every), P, int(every))
    else:
        points = np.asarray(obs_points)
        if points.ndim != 1 or (points.size and not np.issubdtype(points.dtype, np.integer)):
            raise ValueError("obs_points must be a list of integer indices into t")
        if points.size and (points.min() < 0 or points.max() > P - 1):
            raise ValueError(f"obs_points must lie in 0 .. {P - 1} (the points of t)")
        if np.any(np.diff(points) <= 0):
            raise ValueError("obs_points must be strictly increasing")
    if points.size == 0:
        raise ValueError(f"no observation: no observation point on the {P} points of t")
    data = np.asarray(data if data is not None else [], dtype=np.float64)
    if data.shape != (points.shape[0], len(names)):
        raise ValueError(f"data must be [{points.shape[0]}, {len(names)}] (observation points x observed states), got "
                         f"{list(data.shape)}")
    if np.isinf(data).any():
        raise ValueError("data holds an infinite value (a missing measurement is NaN)")
    if np.isnan(data).all():
        raise ValueError("no observation: every entry of data is NaN")
    obs_sd = _per('obs_sd', obs_sd if obs_sd is not None else [], len(names), 'observed state')
    if not np.all(np.isfinite(obs_sd) & (obs_sd > 0)):
        raise ValueError(f"obs_sd must be positive and finite, got {obs_sd.tolist()}")
    return names, points, data, obs_sd


def _prepare_assimilate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
                        obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0,
                        keep=None):
    """``_prepare`` and what the filter adds; touches no device."""
    if keep not in (None, 'particles'):
        raise ValueError("keep must be None or 'particles'")
    p = _prepare(models, states, inputs, forcing, y0, t, draws, bounds, False, None, lds_per_member=False)
    K, E, P = p['K'], p['E'], p['n_steps'] + 1
    names, points, data, obs_sd = _prepare_observations(p['states'], P, observe, data, obs_points, every, obs_sd)
    process_sd = _per('process_sd', 0.0 if process_sd is None else process_sd, K, 'state')
    if not np.all(np.isfinite(process_sd) & (process_sd >= 0)):
        raise ValueError(f"process_sd must be non-negative and finite, got {process_sd.tolist()}")
    y0_sd = _per('y0_sd', 0.0 if y0_sd is None else y0_sd, K, 'state')
    if not np.all(np.isfinite(y0_sd) & (y0_sd >= 0)):
        raise ValueError(f"y0_sd must be non-negative and finite, got {y0_sd.tolist()}")
    if not 0.0 <= float(resample_below) <= 1.0:
        raise ValueError(f"resample_below must lie in [0, 1] (a fraction of the {PARTICLES} particles), got {resample_below}")
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    n_lane_rows = 1 + p['fac_norm'].shape[0] + (p['norm_src'].shape[0] - p['n_norm_forcing'])
    n_coef = p['coef'].shape[0]
    lds_bytes = (n_lane_rows + 1) * LANES * 8 + n_coef * 8
    if lds_bytes > LDS_BUDGET:
        raise ValueError(f"the system needs {lds_bytes} bytes of LDS (({n_lane_rows} factor and state rows + the exchange "
                         f"row) x {LANES} x 8 + {n_coef} coefficients x 8), a wavefront has {LDS_BUDGET}")
    obs_row = np.full(P, -1, dtype=np.int32)
    obs_row[points] = np.arange(points.shape[0], dtype=np.int32)
    log_scale = [float(np.log(sd * np.sqrt(2.0 * np.pi))) for sd in obs_sd]
    obs_const = np.zeros(points.shape[0])
    for r in range(points.shape[0]):
        for o in range(len(names)):
            if not np.isnan(data[r, o]):
                obs_const[r] = obs_const[r] + log_scale[o]
    n_rows = np.atleast_2d(np.asarray(_model_fields(models[0], 0)['betas'])).shape[0]
    p.update(obs_state=np.array([p['states'].index(name) for name in names], dtype=np.int32), obs_sd=obs_sd,
             obs_points=points.astype(np.int64), obs_row=obs_row, data=np.ascontiguousarray(data), obs_const=obs_const,
             process_q=process_sd * np.sqrt(p['h']), y0_sd=y0_sd, threshold=float(resample_below) * PARTICLES,
             seed=int(seed) & 0xFFFFFFFF, draw_ids=_draw_ids(n_rows, draws, E), want_particles=keep == 'particles',
             lds_bytes=lds_bytes)
    return p


def _run_assimilate_host(p, normal_hook=None):
    """-> (stats [E, n_obs, 2 K + 3], particles [E, n_obs, 64, K], weights [E, n_obs, 64], first_saturation, collapsed):
    the rows of fokl_assimilate_ensemble.  ``normal_hook`` (tests) maps every array of normals before it is used."""
    K, E, S, N = p['K'], p['E'], p['n_steps'], PARTICLES
    ids, seed = p['draw_ids'], p['seed']
    n_obs = p['data'].shape[0]
    wide = dict(p, coef=np.repeat(p['coef'], N, axis=1))              # member e * 64 + i is particle i of draw e
    normals = (lambda z: z) if normal_hook is None else normal_hook
    z = normals(_capi.assimilate_rng(seed, ids, 0, _capi.ASSIMILATE_INIT, N * K)).reshape(E, K, N)
    y = np.ascontiguousarray((p['y0'][:, :, np.newaxis] + p['y0_sd'][:, np.newaxis, np.newaxis] * z.transpose(1, 0, 2))
                             .reshape(K, E * N))
    W = np.full((E, N), 1.0 / N)
    stats = np.zeros((E, n_obs, 2 * K + 3))
    particles, weights = np.empty((E, n_obs, N, K)), np.empty((E, n_obs, N))
    first, collapsed = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    fac = np.ones((1 + p['fac_norm'].shape[0], E * N))
    xn = np.zeros((p['norm_src'].shape[0], E * N))

    def observe(point, r, W, collapsed):
        Y = y.reshape(K, E, N)                                        # a view: the gather below writes the particles
        row = p['data'][r]
        present = np.flatnonzero(~np.isnan(row))
        increment, alive = np.zeros(E), np.ones(E, dtype=bool)
        if present.size:
            ss = np.zeros((E, N))
            for o in present:
                dev = (row[o] - Y[p['obs_state'][o]]) / p['obs_sd'][o]
                ss = ss + dev * dev
            lw = -0.5 * ss
            m = lane_max(lw)
            with np.errstate(all='ignore'):
                g = W * np.exp(lw - m[:, np.newaxis])
                G = lane_sum(g)
                alive = (G > 0.0) & (G < np.inf) & (m >= LW_FLOOR)
                W = np.where(alive[:, np.newaxis], g / G[:, np.newaxis], 1.0 / N)
                increment = np.where(alive, (m + np.log(G)) - p['obs_const'][r], -np.inf)
            collapsed = np.where((collapsed < 0) & ~alive, np.int32(r), collapsed).astype(np.int32)
        with np.errstate(all='ignore'):
            ess = 1.0 / lane_sum(W * W)
            for j in range(K):
                mu = lane_sum(W * Y[j])
                dev = Y[j] - mu[:, np.newaxis]
                stats[:, r, j], stats[:, r, K + j] = mu, lane_sum(W * (dev * dev))
        particles[:, r], weights[:, r] = Y.transpose(1, 2, 0), W
        resample = alive & (ess < p['threshold']) if present.size else np.zeros(E, dtype=bool)
        stats[:, r, 2 * K], stats[:, r, 2 * K + 1], stats[:, r, 2 * K + 2] = ess, increment, resample
        if resample.any():
            u = _capi.assimilate_rng(seed, ids, point, _capi.ASSIMILATE_RESAMPLE, 1)[:, 0]
            ancestors = systematic_ancestors(W, u)
            W = W.copy()
            for e in np.flatnonzero(resample):
                Y[:, e, :] = Y[:, e, ancestors[e]]
                W[e] = 1.0 / N
        return W, collapsed

    if p['obs_row'][0] >= 0:
        W, collapsed = observe(0, p['obs_row'][0], W, collapsed)
    for s in range(S):
        with np.errstate(all='ignore'):
            y, acted = _step(wide, fac, xn, y, s)
        y = np.ascontiguousarray(y)
        for j in range(K):
            if p['process_q'][j] != 0.0:
                z = normals(_capi.assimilate_rng(seed, ids, s + 1, j, N))
                y[j] = y[j] + (p['process_q'][j] * z).reshape(E * N)
        first = np.where((first < 0) & acted.reshape(E, N).any(axis=1), np.int32(s), first).astype(np.int32)
        if p['obs_row'][s + 1] >= 0:
            W, collapsed = observe(s + 1, p['obs_row'][s + 1], W, collapsed)
    return stats, particles, weights, first, collapsed


def _draw_weights(log_evidence):
    """exp(log_evidence) normalised over the draws (axis 0); uniform where every draw is -inf."""
    top = np.max(log_evidence, axis=0, keepdims=True)
    with np.errstate(all='ignore'):
        w = np.exp(log_evidence - np.where(np.isfinite(top), top, 0.0))
        total = np.sum(w, axis=0, keepdims=True)
        return np.where(total > 0, w / total, 1.0 / log_evidence.shape[0])


def _assemble_assimilate(p, stats, particles, weights, first, collapsed):
    K, E = p['K'], p['E']
    draw_mean, draw_var = stats[:, :, :K].transpose(0, 2, 1).copy(), stats[:, :, K:2 * K].transpose(0, 2, 1).copy()
    ess, increment, resampled = stats[:, :, 2 * K].copy(), stats[:, :, 2 * K + 1], stats[:, :, 2 * K + 2] != 0
    log_evidence = np.cumsum(increment, axis=1)                       # in observation order; -inf stays -inf
    running = _draw_weights(log_evidence)                             # [E, n_obs]
    w = running[:, np.newaxis, :]
    with np.errstate(all='ignore'):
        mean = np.sum(np.where(w > 0, w * draw_mean, 0.0), axis=0)
        spread = draw_var + (draw_mean - mean[np.newaxis]) * (draw_mean - mean[np.newaxis])
        sd = np.sqrt(np.sum(np.where(w > 0, w * spread, 0.0), axis=0))
    final = running[:, -1].copy()
    u = float(_capi.assimilate_rng(p['seed'], np.zeros(1, dtype=np.uint32), 0, _capi.ASSIMILATE_DRAW_INDEX, 1)[0, 0])
    c = np.cumsum(final)
    chosen = np.minimum(np.searchsorted(c, (np.arange(E) + u) / E * c[-1], side='right'), E - 1)
    res = SimulateResult(t_obs=p['T'][p['obs_points']], mean=mean, sd=sd, draw_mean=draw_mean, draw_var=draw_var,
                         log_evidence=log_evidence, weights=final, ess_draws=float(1.0 / np.sum(final * final)),
                         draw_index=p['draw_ids'][chosen].astype(np.int64), ess=ess, resampled=resampled,
                         first_saturation=first, collapsed=collapsed, states=list(p['states']))
    if p['want_particles']:
        res['particles'], res['particle_weights'] = particles, weights
        n_obs = particles.shape[1]
        band = np.empty((K, n_obs, 2))
        for k in range(n_obs):
            joint = (running[:, k, np.newaxis] * weights[:, k]).ravel()
            for j in range(K):
                values = particles[:, k, :, j].ravel()
                order = np.argsort(values, kind='stable')
                cumulative = np.cumsum(joint[order])
                cumulative = cumulative / cumulative[-1]
                for side, level in enumerate((0.025, 0.975)):
                    band[j, k, side] = values[order[min(int(np.searchsorted(cumulative, level)), values.shape[0] - 1)]]
        res['bounds'] = band
    return res


_ASSIMILATE_SIGNATURE = """
    models, states, inputs, forcing, y0, t, draws, bounds : as for ``simulate``.  Draw e's random numbers are keyed by the
                  row of ``betas`` it selects, so a subset of the draws reproduces the full run's ('mean': id 0; the
                  members of an initial-condition sweep of one draw: 0 .. E - 1)
    observe     : the names of the measured states
    data        : [n_obs, len(observe)] in true scale; NaN is a missing measurement, a row of NaN weighs nothing
    obs_points  : strictly increasing indices into the points of ``t`` (0 .. P - 1), one per row of ``data``; or
    every       : k, for the points k, 2k, ... -- exactly one of the two
    obs_sd      : the measurement noise's standard deviation per observed state (positive)
    process_sd  : per state and per square root of a time unit: a step adds process_sd[j] sqrt(h) z (default 0)
    y0_sd       : per state, the spread of the particles at point 0 (default 0)
    resample_below : resample where the particles' ESS falls below this fraction of 64 (0: never, 1: wherever ESS < 64)
    seed        : of the filter's own counter-based random numbers; numpy's stream, ``setnos`` and the fits are left alone
    keep        : 'particles' also returns the particles and their weights (before resampling) and ``bounds``

    Returns a ``SimulateResult`` (a dict with attribute access): t_obs [n_obs]; mean, sd [n_states, n_obs] pooled over the
    draws with the running draw weights; draw_mean, draw_var [E, n_states, n_obs]; log_evidence [E, n_obs] cumulative;
    weights [E] = exp(log_evidence[:, -1]) normalised, ess_draws = 1 / sum(weights^2); draw_index [E] rows of ``betas``
    drawn proportional to ``weights`` (systematic, from ``seed``), usable as ``draws=``; ess [E, n_obs] before resampling,
    resampled [E, n_obs] bool; first_saturation [E] int32 (the first step in which a clamp or the slope rule acted for any
    particle, -1: never), collapsed [E] int32 (the first observation at which no particle had a positive weight, -1:
    never); with keep='particles' particles [E, n_obs, 64, n_states], particle_weights [E, n_obs, 64] and bounds
    [n_states, n_obs, 2], the weighted 2.5 % / 97.5 % quantiles over (draw, particle)."""


def assimilate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
               obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0, keep=None,
               device=None):
    """Filter a system of fitted models against measurements, one particle filter per posterior draw, on the device
    (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_assimilate(models, states, inputs, forcing, y0, t, draws, bounds, observe, data, obs_points, every, obs_sd,
                            process_sd, y0_sd, resample_below, seed, keep)
    ctx = _device_context(device)
    return _assemble_assimilate(p, *ctx.assimilate_ensemble(p))


def assimilate_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, observe=None, data=None,
                    obs_points=None, every=None, obs_sd=None, process_sd=None, y0_sd=None, resample_below=0.5, seed=0,
                    keep=None, normal_hook=None):
    """``assimilate`` in numpy on this host, vectorised over (draws, particles): the statement the kernel is tested
    against (module docstring), not a fallback.  Same arguments, same result fields; ``normal_hook`` (tests) maps every
    array of normals before it is used."""
    p = _prepare_assimilate(models, states, inputs, forcing, y0, t, draws, bounds, observe, data, obs_points, every, obs_sd,
                            process_sd, y0_sd, resample_below, seed, keep)
    return _assemble_assimilate(p, *_run_assimilate_host(p, normal_hook))


assimilate.__doc__ += _ASSIMILATE_SIGNATURE
assimilate_host.__doc__ += _ASSIMILATE_SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# control: projected Gauss-Newton on a least-squares cost, per posterior draw (module docstring)
# ---------------------------------------------------------------------------------------------------------

from .optimize import (start_points, CONVERGED, ITERATION_LIMIT, NON_FINITE, STALLED, STATUS_TEXT,   # noqa: E402,F401
                       ARMIJO, NOISE, PIVOT_FLOOR, MAX_SOLVES)

CONTROL_MAX_DECISIONS = 32                # D = controls x segments: one direction lane each, the Newton trials fill lanes 0 .. 30
CONTROL_MAX_STEPS = 4096                  # two passes over the horizon are one launch
CONTROL_TRIALS = 31                       # alpha = 1, 1/2, ..., 2**-30 in lanes i (Newton) and 32 + i (steepest descent)
_TRIAL_ALPHA = np.ldexp(1.0, -np.arange(CONTROL_TRIALS))


def control_lds_bytes(n_factors, n_norm_state, n_coef, D):
    """LDS bytes of a solve's wavefront: values and tangents of slot 0, the factors and the normalised states as
    [item][lane], four rows of 64 (exchange, z, g, direction), row d of H (afterwards the trial points) as [D][64], and
    the draw's coefficients once."""
    return (2 * (1 + n_factors + n_norm_state) + 4 + D) * LANES * 8 + n_coef * 8


def _named(name, given, states, what, default):
    out = np.full(len(states), float(default))
    for key, value in dict(given or {}).items():
        if str(key) not in states:
            raise ValueError(f"{name}: '{key}' is not a state ({states})")
        out[states.index(str(key))] = what(key, value)
    return out


def _column_box(p, readers, name, given, option, what):
    """(lo, hi) of an input column the caller chooses (a control, a calibrated parameter): the intersection of the training
    ranges of the normalised inputs ``readers`` that read it, or ``given[name]`` inside that range (``option`` names the
    argument, ``what`` the column's role in the messages)."""
    range_lo, range_hi = np.max(p['norm_lo'][readers]), np.min(p['norm_hi'][readers])
    if name in given:
        pair = np.asarray(given[name], dtype=np.float64)
        if pair.shape != (2,) or not np.isfinite(pair).all():
            raise ValueError(f"{option}['{name}'] must be two finite numbers (lo, hi) in true scale")
        lo, hi = pair
        if not lo < hi:
            raise ValueError(f"{option}['{name}'] is empty (lower {lo}, upper {hi})")
        for n in readers:
            if (lo - p['norm_lo'][n]) / p['norm_span'][n] < -1e-12 or (hi - p['norm_lo'][n]) / p['norm_span'][n] > 1 + 1e-12:
                raise ValueError(f"{option}['{name}'] reaches outside the training range [{range_lo}, {range_hi}] "
                                 f"of the columns that read it: the models are not extrapolated")
    else:
        lo, hi = range_lo, range_hi
        if not lo < hi:
            raise ValueError(f"{what} '{name}': its box is empty, the training ranges of the columns that read it have "
                             f"no interval in common")
    return float(lo), float(hi)


def _prepare_control(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds, targets,
                     weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter, tol, keep):
    """``_prepare`` with the controls as forcing columns, and what the solver adds; touches no device."""
    wanted = {keep} if isinstance(keep, str) else set(keep or ())
    if not wanted <= {'members', 'all'}:
        raise ValueError("keep must be None, 'members', 'all' or a list of the two")
    controls = [str(name) for name in (controls if controls is not None else [])]
    if not controls:
        raise ValueError("controls must name at least one input column the solver chooses")
    if len(set(controls)) != len(controls):
        raise ValueError(f"controls names a column twice: {controls}")
    forcing = dict(forcing or {})
    state_names = [str(name) for name in states]
    for name in controls:
        if name in state_names:
            raise ValueError(f"controls: '{name}' is a state")
        if name in [str(key) for key in forcing]:
            raise ValueError(f"controls: '{name}' is a forcing key")
    start, stop, h = (float(v) for v in t)
    if not (np.isfinite([start, stop, h]).all() and h > 0):
        raise ValueError("t = (start, stop, h) needs finite numbers and h > 0")
    n_steps = len(np.arange(start, stop + h, h)) - 1
    if n_steps < 1:
        raise ValueError("control needs at least one step: t = (start, stop, h) holds no step at all")
    if n_steps > CONTROL_MAX_STEPS:
        raise ValueError(f"control handles at most {CONTROL_MAX_STEPS} steps per call, t holds {n_steps}: shorten the horizon "
                         f"or recede it")
    placeholder = np.zeros(n_steps)
    p = _prepare(models, states, inputs, {**forcing, **{name: placeholder for name in controls}}, y0, t, draws, bounds, False,
                 None, lds_per_member=False)
    NS, E, P = p['K'], p['E'], n_steps + 1
    states = p['states']
    nc = len(controls)
    col_control = np.full(len(p['forcing_cols']), -1, dtype=np.int32)
    for c, name in enumerate(controls):
        if name not in p['forcing_cols']:
            raise ValueError(f"controls: no model reads '{name}' (no term of any model has an order on it)")
        col_control[p['forcing_cols'].index(name)] = c

    # ---- segments ----
    if np.ndim(segments) == 0:
        if int(segments) != segments or int(segments) < 1:
            raise ValueError("segments must be a positive count or an increasing array of first steps that begins with 0")
        hold = -(-n_steps // int(segments))
        seg_first = np.arange(0, n_steps, hold)
        if len(seg_first) != int(segments):
            raise ValueError(f"segments={int(segments)} holds of ceil({n_steps} / {int(segments)}) = {hold} steps cover the "
                             f"{n_steps} steps in {len(seg_first)}: ask for at most that many")
    else:
        seg_first = np.asarray(segments)
        if seg_first.ndim != 1 or seg_first.size == 0 or not np.issubdtype(seg_first.dtype, np.integer) or seg_first[0] != 0 \
                or np.any(np.diff(seg_first) <= 0) or seg_first[-1] >= n_steps:
            raise ValueError(f"segments as an array must hold increasing first steps, beginning with 0 and below {n_steps}")
    Kseg = int(len(seg_first))
    D = nc * Kseg
    if D > CONTROL_MAX_DECISIONS:
        raise ValueError(f"{nc} controls x {Kseg} segments = {D} decision values, the solver handles at most "
                         f"{CONTROL_MAX_DECISIONS}")
    seg_of = (np.searchsorted(seg_first, np.arange(n_steps), side='right') - 1).astype(np.int32)

    # ---- the control box: inside the training range of every column that reads the control ----
    norm_control = np.array([col_control[-(src + 1)] for src in p['norm_src'][:p['n_norm_forcing']]], dtype=np.int32)
    given = {str(key): value for key, value in dict(control_bounds or {}).items()}
    for name in given:
        if name not in controls:
            raise ValueError(f"control_bounds: '{name}' is not a control ({controls})")
    lo, hi = np.empty(nc), np.empty(nc)
    for c, name in enumerate(controls):
        lo[c], hi[c] = _column_box(p, np.flatnonzero(norm_control == c), name, given, 'control_bounds', 'control')
    width = hi - lo

    # ---- the cost ----
    def number(name):
        def check(key, value):
            if np.ndim(value) != 0 or not np.isfinite(value) or float(value) < 0:
                raise ValueError(f"{name}['{key}'] must be a non-negative finite number (negative weights are refused)")
            return float(value)
        return check
    ref = np.full((NS, P), np.nan)
    for key, value in dict(targets or {}).items():
        if str(key) not in states:
            raise ValueError(f"targets: '{key}' is not a state ({states})")
        value = np.asarray(value, dtype=np.float64)
        if value.ndim == 0:
            value = np.full(P, float(value))
        if value.shape != (P,):
            raise ValueError(f"targets['{key}'] must be a number or one value per point of t ({P}), got shape {list(value.shape)}")
        if np.isinf(value).any():
            raise ValueError(f"targets['{key}'] holds an infinite value (a point that is not tracked is NaN)")
        ref[states.index(str(key))] = value
    targeted = ~np.isnan(ref).all(axis=1)
    w = _named('weights', weights, states, number('weights'), np.nan)
    w = np.where(np.isnan(w), np.where(targeted, 1.0, 0.0), w)
    term = _named('terminal', terminal, states, number('terminal'), 0.0)
    for j in np.flatnonzero(term > 0):
        if np.isnan(ref[j, P - 1]):
            raise ValueError(f"terminal['{states[j]}'] needs a target at the last point")
    lim_lo, lim_hi = np.full(NS, -np.inf), np.full(NS, np.inf)
    for key, pair in dict(limits or {}).items():
        if str(key) not in states:
            raise ValueError(f"limits: '{key}' is not a state ({states})")
        if np.ndim(pair) != 1 or len(pair) != 2:
            raise ValueError(f"limits['{key}'] must be (lower, upper); None leaves a side open")
        low, high = (None if v is None else float(v) for v in pair)
        if (low is not None and not np.isfinite(low)) or (high is not None and not np.isfinite(high)) or \
                (low is not None and high is not None and not low <= high):
            raise ValueError(f"limits['{key}'] must be finite with lower <= upper; None leaves a side open")
        j = states.index(str(key))
        lim_lo[j], lim_hi[j] = (-np.inf if low is None else low), (np.inf if high is None else high)
    if np.ndim(limit_weight) != 0 or not np.isfinite(limit_weight) or limit_weight < 0:
        raise ValueError("limit_weight must be a non-negative finite number (negative weights are refused)")
    move = np.zeros(nc)
    for key, value in dict(move_weight or {}).items():
        if str(key) not in controls:
            raise ValueError(f"move_weight: '{key}' is not a control ({controls})")
        move[controls.index(str(key))] = number('move_weight')(key, value)
    has_previous = previous is not None
    prev = np.zeros(nc)
    if has_previous:
        prev = np.asarray(previous, dtype=np.float64)
        if prev.shape != (nc,) or not np.isfinite(prev).all():
            raise ValueError(f"previous must be [{nc}] finite numbers (one value per control, true scale), got shape "
                             f"{list(np.shape(previous))}")
    wt = p['h'] * w
    hl = p['h'] * float(limit_weight)
    tracked = np.any((wt[:, np.newaxis] > 0) & ~np.isnan(ref[:, 1:]))
    limited = hl > 0 and (np.isfinite(lim_lo).any() or np.isfinite(lim_hi).any())
    penalised = np.any(move > 0) and (Kseg > 1 or has_previous)
    if not (tracked or np.any(term > 0) or limited or penalised):
        raise ValueError("the cost has no residual at all: nothing is tracked, limited or penalised")

    # ---- starts ----
    if np.ndim(starts) != 0 or int(starts) != starts or int(starts) < 1:
        raise ValueError("starts must be a count >= 1")
    S = int(starts)
    if E * S > MAX_SOLVES:
        raise ValueError(f"{E} draws x {S} starts: one call runs at most {MAX_SOLVES} solves")
    z0 = np.full((S, nc, Kseg), 0.5)
    if init is not None:
        first = np.asarray(init, dtype=np.float64)
        if first.shape != (nc, Kseg) or not np.isfinite(first).all():
            raise ValueError(f"init must be [{nc}, {Kseg}] finite numbers (controls x segments, true scale), got shape "
                             f"{list(np.shape(init))}")
        z0[0] = (first - lo[:, np.newaxis]) / width[:, np.newaxis]
    if S > 1:
        z0[1:] = ((start_points(S - 1, lo, hi) - lo) / width)[:, :, np.newaxis]
    z0 = np.minimum(np.maximum(z0, 0.0), 1.0).reshape(S, D)
    if int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError("max_iter must be a non-negative integer")
    if not (tol >= 0):
        raise ValueError("tol must be >= 0")
    n_norm_state = p['norm_src'].shape[0] - p['n_norm_forcing']
    lds_bytes = control_lds_bytes(p['fac_norm'].shape[0], n_norm_state, p['coef'].shape[0], D)
    if lds_bytes > LDS_BUDGET:
        raise ValueError(f"the system needs {lds_bytes} bytes of LDS ((2 x (1 + {p['fac_norm'].shape[0]} factors + {n_norm_state} "
                         f"normalised states) + 4 + {D} decision values) x {LANES} x 8 + {p['coef'].shape[0]} coefficients x 8), "
                         f"a wavefront has {LDS_BUDGET}")
    p.update(controls=controls, n_controls=nc, segments=Kseg, D=D, seg_first=seg_first.astype(np.int32), seg_of=seg_of,
             col_control=col_control, norm_control=norm_control, ctl_lo=lo, ctl_width=width, ref=np.ascontiguousarray(ref),
             wt=wt, term=term, lim_lo=lim_lo, lim_hi=lim_hi, hl=hl, move=move, prev=prev, has_previous=bool(has_previous),
             z0=np.ascontiguousarray(z0), starts=S, max_iter=int(max_iter), tol=float(tol), want_members='members' in wanted,
             want_all='all' in wanted, lds_bytes=lds_bytes)
    return p


def _clip01(x):
    x = np.where(x < 0.0, 0.0, x)
    return np.where(x > 1.0, 1.0, x)


def _factor_dual(p, f, v):
    """Factor f at normalised v [M] -> (value as ``_factor_values`` forms it, d value / d v)."""
    if p['fac_kind'][f] == SPLINE:
        pieces = p['spline_table'][p['fac_row'][f]]
        q = np.ceil(v * 499.0)
        q = q + (q == 0)
        q = q - 1
        s = 499.0 * v - q
        c = pieces[np.clip(np.where(np.isfinite(q), q, 0.0), 0, PIECES - 1).astype(np.intp)]
        q2 = c[..., 2] + s * c[..., 3]
        q1 = c[..., 1] + s * q2
        d1 = q2 + s * c[..., 3]
        d0 = q1 + s * d1
        return c[..., 0] + s * q1, 499.0 * d0
    c = p['bern_table'][p['fac_row'][f]]
    degree = int(p['fac_degree'][f])
    value, slope = np.full(v.shape, float(c[degree])), np.zeros(v.shape)
    for k in range(degree - 1, -1, -1):
        slope = slope * v + value
        value = value * v + float(c[k])
    return value, slope


def _control_pass(p, z, member, tangents=False, record=False):
    """One pass over the horizon for M solves / trial points: z [D, M], ``member`` [M] the draw of each.  Returns a dict with
    F and noise [M]; with ``tangents`` also g [D, M] and H [D, D, M] (entry [d, d'] as lane d forms it); with ``record``
    members [M, n_states, P] and first [M].  The module docstring states every operation."""
    NS, S, M, D, Kseg = p['K'], p['n_steps'], z.shape[1], p['D'], p['segments']
    h, nF, nN, nNF, nFF = p['h'], p['fac_norm'].shape[0], p['norm_src'].shape[0], p['n_norm_forcing'], p['n_forcing_factors']
    cf, y = p['coef'][:, member], p['y0'][:, member].copy()
    fac, xn = np.ones((1 + nF, M)), np.zeros((nN, M))
    F, noise = np.zeros(M), np.zeros(M)
    first = np.full(M, -1, dtype=np.int32)
    members = np.empty((M, NS, S + 1)) if record else None
    if record:
        members[:, :, 0] = y.T
    if tangents:
        tfac, txn, ty = np.zeros((1 + nF, D, M)), np.zeros((nN, D, M)), np.zeros((NS, D, M))
        g, H = np.zeros((D, M)), np.zeros((D, D, M))
    zero = np.zeros((D, M)) if tangents else None

    def residual(weight, a, b, t, act=None):
        nonlocal F, noise, g, H
        r, mag = a - b, np.abs(a) + np.abs(b)
        if act is not None:
            r, mag = np.where(act, r, 0.0), np.where(act, mag, 0.0)
        q = weight * r
        F = F + q * r
        noise = noise + weight * (mag * mag)
        if tangents:
            if act is not None:
                t = np.where(act, t, 0.0)
            g = g + (2.0 * q) * t
            H = H + ((2.0 * weight) * t)[:, np.newaxis, :] * t[np.newaxis, :, :]

    def factors(begin, end):
        for f in range(begin, end):
            n = p['fac_norm'][f]
            if tangents:
                fac[f + 1], slope = _factor_dual(p, f, xn[n])
                tfac[f + 1] = slope * txn[n]
            elif p['fac_kind'][f] == SPLINE:
                fac[f + 1] = spline_value(p['spline_table'][p['fac_row'][f]], xn[n])
            else:
                fac[f + 1] = bernoulli_value(p['bern_table'][p['fac_row'][f], :p['fac_degree'][f] + 1], xn[n])

    def stage(at, tat):
        acted = np.zeros(M, dtype=bool)
        for n in range(nNF, nN):
            j = p['norm_src'][n]
            xn[n], clamp = _clamped((at[j] - p['norm_lo'][n]) / p['norm_span'][n])
            acted |= clamp
            if tangents:
                txn[n] = np.where(clamp, 0.0, tat[j] / p['norm_span'][n])
        factors(nFF, nF)
        dy = np.empty((NS, M))
        tdy = np.empty((NS, D, M)) if tangents else None
        for k in range(NS):
            delta, phi = np.zeros(M), np.ones(M)
            tdelta, tphi = zero, zero
            for a, b, c, w in p['entries'][p['entry_begin'][k]:p['entry_begin'][k] + p['entry_count'][k]]:
                for slot in (a, b, c):
                    if tangents:
                        tphi = tphi * fac[slot] + phi * tfac[slot]
                    phi = phi * fac[slot]
                if w >= 0:
                    delta = delta + cf[w] * phi
                    phi = np.ones(M)
                    if tangents:
                        tdelta = tdelta + cf[w] * tphi
                        tphi = zero
            s = (delta + cf[p['constant'][k]]) * h
            out = ((at[k] >= p['box'][k, 1]) & (s > 0)) | ((at[k] <= p['box'][k, 0]) & (s < 0))
            dy[k] = np.where(out, 0.0, s)
            if tangents:
                tdy[k] = np.where(out, 0.0, tdelta * h)
            acted |= out
        return dy, tdy, acted

    with np.errstate(all='ignore'):
        for s in range(S):
            k = p['seg_of'][s]
            acted = np.zeros(M, dtype=bool)
            for n in range(nNF):
                col = -(p['norm_src'][n] + 1)
                c = p['col_control'][col]
                x = np.full(M, p['forcing'][s, col]) if c < 0 else p['ctl_lo'][c] + z[c * Kseg + k] * p['ctl_width'][c]
                xn[n], clamp = _clamped((x - p['norm_lo'][n]) / p['norm_span'][n])
                acted |= clamp
                if tangents:
                    txn[n] = 0.0
                    if c >= 0:
                        txn[n, c * Kseg + k] = np.where(clamp, 0.0, p['ctl_width'][c] / p['norm_span'][n])
            factors(0, nFF)
            dy = tdy = total = ttotal = None
            for st in range(4):
                reach, weight = (1.0 if st == 3 else 0.5), (2.0 if st in (1, 2) else 1.0)
                at = y if st == 0 else y + dy * reach
                tat = None if not tangents else ty if st == 0 else ty + tdy * reach
                dy, tdy, stage_acted = stage(at, tat)
                total = dy if st == 0 else total + weight * dy
                if tangents:
                    ttotal = tdy if st == 0 else ttotal + weight * tdy
                acted |= stage_acted
            y = y + total / 6
            if tangents:
                ty = ty + ttotal / 6
            if record:
                members[:, :, s + 1] = y.T
                first = np.where((first < 0) & acted, np.int32(s), first).astype(np.int32)
            point = s + 1
            for j in range(NS):
                t = ty[j] if tangents else None
                target = p['ref'][j, point]
                if p['wt'][j] > 0 and not np.isnan(target):
                    residual(p['wt'][j], y[j], target, t)
                if point == S and p['term'][j] > 0:
                    residual(p['term'][j], y[j], target, t)
                if p['hl'] > 0 and p['lim_hi'][j] < np.inf:
                    residual(p['hl'], y[j], p['lim_hi'][j], t, y[j] > p['lim_hi'][j])
                if p['hl'] > 0 and p['lim_lo'][j] > -np.inf:
                    residual(p['hl'], p['lim_lo'][j], y[j], -t if tangents else None, y[j] < p['lim_lo'][j])
        for c in range(p['n_controls']):
            if not p['move'][c] > 0:
                continue
            for k in range(Kseg):
                if k == 0 and not p['has_previous']:
                    continue
                d = c * Kseg + k
                t = None
                if tangents:
                    t = np.zeros((D, M))
                    t[d] = p['ctl_width'][c]
                    if k > 0:
                        t[d - 1] = -p['ctl_width'][c]
                now = p['ctl_lo'][c] + z[d] * p['ctl_width'][c]
                before = np.full(M, p['prev'][c]) if k == 0 else p['ctl_lo'][c] + z[d - 1] * p['ctl_width'][c]
                residual(p['move'][c], now, before, t)
    out = dict(F=F, noise=noise)
    if tangents:
        out.update(g=g, H=H)
    if record:
        out.update(members=members, first=first)
    return out


def _control_direction(H, g, active):
    """Step 4: the modified-Cholesky direction of every solve, lane = row.  H [D, D, B] (its lower triangle is read)."""
    D, B = g.shape
    with np.errstate(all='ignore'):
        free = np.zeros(B)
        for j in range(D):
            free = np.where(active[j], free, np.fmax(free, np.abs(H[j, j])))
        floor = PIVOT_FLOOR * np.fmax(1.0, free)
        L = np.zeros((D, D, B))
        for j in range(D):
            for i in range(j, D):
                s = np.where(active[i] | active[j], 1.0 if i == j else 0.0, H[i, j])
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if i == j:
                    s = np.where(s > floor, s, np.fmax(np.abs(s), floor))
                    L[j, j] = np.sqrt(s)
                else:
                    L[i, j] = s / L[j, j]
        s = np.where(active, 0.0, -g)
        for k in range(D):                                            # forward: row k is final once rows 0 .. k - 1 are taken off
            s[k] = s[k] / L[k, k]
            for i in range(k + 1, D):
                s[i] = s[i] - L[i, k] * s[k]
        for k in range(D - 1, -1, -1):                                # back: row k is final once rows D - 1 .. k + 1 are taken off
            s[k] = s[k] / L[k, k]
            for i in range(k):
                s[i] = s[i] - L[k, i] * s[k]
    return s


def _control_solve_host(p):
    """Every (draw, start) solve -> dict(z [E, S, D], cost, cost_start, status, iterations [E, S] and, with max_iter == 0,
    the first tangent pass F [E, S], g [E, S, D], H [E, S, D, D])."""
    E, S, D, max_iter, tol = p['E'], p['starts'], p['D'], p['max_iter'], p['tol']
    B = E * S
    member = np.repeat(np.arange(E), S)
    z = np.ascontiguousarray(np.tile(p['z0'], (E, 1)).T)              # [D, B], solve b = e S + s
    status = np.full(B, -1, dtype=np.int32)
    iterations, descent = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    cost, cost_start = np.full(B, np.nan), np.full(B, np.nan)
    first_pass = None
    lanes = np.arange(CONTROL_TRIALS)
    for it in range(max_iter + 1):
        idx = np.flatnonzero(status < 0)
        if idx.size == 0:
            break
        zi = z[:, idx]
        out = _control_pass(p, zi, member[idx], tangents=True)
        F, g, H, noise = out['F'], out['g'], out['H'], out['noise']
        if it == 0:
            cost_start[idx] = F
            first_pass = dict(F=F.reshape(E, S), g=g.T.reshape(E, S, D), H=H.transpose(2, 0, 1).reshape(E, S, D, D))
        cost[idx] = F
        with np.errstate(all='ignore'):
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)
            pg = np.zeros(idx.size)
            for d in range(D):
                pg = np.fmax(pg, np.abs(_clip01(zi[d] - g[d]) - zi[d]))
        code = np.where(~finite, NON_FINITE, np.where(pg <= tol, CONVERGED, ITERATION_LIMIT if it == max_iter else -1))
        stopped = code >= 0
        status[idx[stopped]], iterations[idx[stopped]] = code[stopped], it
        go = np.flatnonzero(~stopped)
        if go.size == 0:
            continue
        idx, zi, F, g, H, noise = idx[go], zi[:, go], F[go], g[:, go], H[:, :, go], noise[go]
        with np.errstate(all='ignore'):
            active = ((zi <= 0.0) & (g > 0)) | ((zi >= 1.0) & (g < 0))
            direction = _control_direction(H, g, active)
            # lane i: P(z + 2^-i d); lane 31 + i here (32 + i of the wavefront): P(z + 2^-i (-g))
            both = np.stack([direction, -g], axis=1)                                              # [D, 2, n]
            trial = _clip01(zi[:, np.newaxis, np.newaxis, :] + _TRIAL_ALPHA[np.newaxis, np.newaxis, :, np.newaxis] *
                            both[:, :, np.newaxis, :])                                            # [D, 2, 31, n]
            n = idx.size
            flat = np.ascontiguousarray(trial.reshape(D, 2 * CONTROL_TRIALS * n))
            Ft = _control_pass(p, flat, np.tile(member[idx], 2 * CONTROL_TRIALS))['F'].reshape(2, CONTROL_TRIALS, n)
            step = trial - zi[:, np.newaxis, np.newaxis, :]
            slope, moved = np.zeros((2, CONTROL_TRIALS, n)), np.zeros((2, CONTROL_TRIALS, n), dtype=bool)
            for d in range(D):
                slope = slope + g[d] * step[d]
                moved |= np.abs(step[d]) > 0
            ok = moved & (Ft <= (F + ARMIJO * np.where(slope < 0, slope, 0.0)) + NOISE * noise)
        ok = ok.reshape(2 * CONTROL_TRIALS, n)
        any_ok = ok.any(axis=0)
        chosen = np.argmax(ok, axis=0)                                # the first Newton lane, else the first steepest-descent lane
        taken = trial.reshape(D, 2 * CONTROL_TRIALS, n)[:, chosen, np.arange(n)]
        z[:, idx[any_ok]] = taken[:, any_ok]
        descent[idx[any_ok & (chosen >= CONTROL_TRIALS)]] += 1
        status[idx[~any_ok]], iterations[idx[~any_ok]] = STALLED, it
    res = dict(z=z.T.reshape(E, S, D).copy(), cost=cost.reshape(E, S), cost_start=cost_start.reshape(E, S),
               status=status.reshape(E, S), iterations=iterations.reshape(E, S), descent_steps=descent.reshape(E, S))
    if max_iter == 0:
        res['first_pass'] = first_pass
    return res


def _best_start(cost, status):
    key = np.where(np.isfinite(cost) & (status != NON_FINITE), cost, np.inf)
    return np.argmin(key, axis=1)


def _run_control_host(p):
    solved = _control_solve_host(p)
    best = _best_start(solved['cost'], solved['status'])
    zb = np.ascontiguousarray(solved['z'][np.arange(p['E']), best].T)
    out = _control_pass(p, zb, np.arange(p['E']), record=True)
    return solved, best.astype(np.int32), out['members'], out['first']


def _assemble_control(p, solved, best, members, first):
    E, nc, Kseg = p['E'], p['n_controls'], p['segments']
    rows = np.arange(E)
    true_scale = lambda zz: p['ctl_lo'][:, np.newaxis] + zz.reshape(zz.shape[:-1] + (nc, Kseg)) * p['ctl_width'][:, np.newaxis]
    z = solved['z'][rows, best]
    u = true_scale(z)
    res = SimulateResult(u=u, z=z.reshape(E, nc, Kseg), cost=solved['cost'][rows, best], status=solved['status'][rows, best],
                         iterations=solved['iterations'][rows, best], descent_steps=solved['descent_steps'][rows, best], cost_start=solved['cost_start'][rows, best],
                         best_start=best.astype(np.int64), u_mean=u.mean(axis=0), t=p['T'], mean=np.mean(members, axis=0),
                         first_saturation=first, controls=list(p['controls']), states=list(p['states']),
                         segment_first=p['seg_first'].astype(np.int64))
    if E >= 2:
        cut = bounds_cut(E)
        us, ms = np.sort(u, axis=0), np.sort(members, axis=0)
        res['u_bounds'] = np.stack([us[cut], us[E - cut]], axis=-1)
        res['bounds'] = np.stack([ms[cut], ms[E - cut]], axis=-1)
    if p['want_members']:
        res['members'] = members
    if p['want_all']:
        res.update(u_all=true_scale(solved['z']), cost_all=solved['cost'], status_all=solved['status'],
                   iterations_all=solved['iterations'], descent_steps_all=solved['descent_steps'])
    if 'first_pass' in solved:
        res['first_pass'] = solved['first_pass']
    return res


def expand_controls(res, e=None):
    """The controls of a result as ``forcing`` arrays [steps]: draw e's own (``res.u[e]``), or ``u_mean`` if e is None.  A
    result of ``control_pooled`` has one sequence for all draws (``u_mean`` = ``u``) and none per draw."""
    if e is not None and res.get('pooled', False):
        raise ValueError("expand_controls: a pooled result holds one control sequence for all draws (e=None), none per draw")
    u = res['u_mean'] if e is None else res['u'][e]
    n_steps = len(res['t']) - 1
    seg_of = np.searchsorted(res['segment_first'], np.arange(n_steps), side='right') - 1
    return {name: u[c][seg_of] for c, name in enumerate(res['controls'])}


_CONTROL_SIGNATURE = """
    models, states, inputs, forcing, y0, t, draws, bounds : as for ``simulate``; ``y0`` [E, n_states] and ``draws=`` take
                  ``assimilate``'s ``draw_mean[:, :, -1]`` and ``draw_index``
    controls    : names of input columns that are neither states nor keys of ``forcing``: the solver chooses their values
    segments    : K, for K holds of ceil(steps / K) steps (the last may be shorter), or an increasing array of first steps
                  that begins with 0
    control_bounds : {control: (lo, hi)} in true scale; default and outer limit: the intersection of the training ranges of
                  the columns that read the control
    targets     : {state: a number or [points]}; NaN: that point is not tracked.  weights {state: w >= 0} (default 1 for a
                  targeted state), terminal {state: w >= 0} on the last point
    limits      : {state: (lower, upper)}, None leaves a side open; soft, weighted by ``limit_weight``
    move_weight : {control: w >= 0} on u_k - u_(k-1); ``previous`` [n_controls] is u before step 0 (without it the first
                  move is free)
    init        : [n_controls, K] start 0 in true scale (default: the box centre); ``starts`` - 1 further starts hold every
                  control constant at the points of ``optimize.start_points``.  Nothing is drawn at random
    max_iter, tol : iteration limit of a solve; projected-gradient tolerance in z.  max_iter=0 evaluates the first tangent
                  pass only and returns it as ``first_pass`` (F [E, S], g [E, S, D], H [E, S, D, D], lower triangle)
    keep        : 'members' also returns every draw's trajectory under its own controls, 'all' every start's solve; a list
                  of both is accepted

    Returns a ``SimulateResult``: u [E, n_controls, K] (true scale, = lo + z (hi - lo)), z, cost, status, iterations,
    cost_start, best_start, descent_steps (iterations whose accepted trial was a steepest-descent lane) [E] of each
    draw's best start (status: ``optimize.STATUS_TEXT``); u_mean [n_controls, K] and, for
    E >= 2, u_bounds [n_controls, K, 2] and bounds [n_states, P, 2] (``evaluate``'s order statistics over the draws); t,
    mean [n_states, P] and first_saturation [E] of the trajectories under each draw's OWN controls; members [E, n_states,
    P] with keep='members'; u_all, cost_all, status_all, iterations_all [E, S, ...] with keep='all'.
    ``expand_controls(res, e)`` gives the controls as ``forcing`` arrays for ``simulate``."""


def control(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None, segments=8,
            control_bounds=None, targets=None, weights=None, terminal=None, limits=None, limit_weight=1e3, move_weight=None,
            previous=None, init=None, starts=1, max_iter=60, tol=1e-10, keep=None, device=None):
    """Which inputs make the states of a fitted system do what is wanted?  One bounded least-squares solve per posterior
    draw and start, every solve a wavefront on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_control(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds, targets,
                         weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter, tol, keep)
    ctx = _device_context(device)
    return _assemble_control(p, *ctx.control_solve(p))


def control_host(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None, segments=8,
                 control_bounds=None, targets=None, weights=None, terminal=None, limits=None, limit_weight=1e3,
                 move_weight=None, previous=None, init=None, starts=1, max_iter=60, tol=1e-10, keep=None):
    """``control`` in numpy on this host, vectorised over solves and trial points: the statement the kernel is tested
    against (module docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare_control(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds, targets,
                         weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter, tol, keep)
    return _assemble_control(p, *_run_control_host(p))


control.__doc__ += _CONTROL_SIGNATURE
control_host.__doc__ += _CONTROL_SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# control_pooled: one control sequence for the whole posterior, the expected cost over the draws (module docstring)
# ---------------------------------------------------------------------------------------------------------

POOL_CHUNK = 64                           # draws per chunk of the pooled sum


def pooled_sum(X, w):
    """sum_e w[e] X[e] over the first axis in the one order the module docstring states: chunks of ``POOL_CHUNK``
    consecutive draws, inside a chunk acc = acc + w_e X_e in index order from 0.0, the chunk sums added in chunk order from
    the first; a draw with w_e == 0 is skipped entirely.  X [E, ...], w [E] -> [...]."""
    X, w = np.asarray(X, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if w.ndim != 1 or X.ndim < 1 or X.shape[0] != w.shape[0]:
        raise ValueError(f"pooled_sum: X must hold one row per weight ({list(w.shape)}), got shape {list(X.shape)}")
    total = None
    with np.errstate(all='ignore'):
        for begin in range(0, w.shape[0], POOL_CHUNK):
            acc = np.zeros(X.shape[1:])
            for e in range(begin, min(begin + POOL_CHUNK, w.shape[0])):
                if w[e] == 0:
                    continue
                acc = acc + w[e] * X[e]
            total = acc if total is None else total + acc
    return np.zeros(X.shape[1:]) if total is None else total


def _pool_weights(draw_weights, E):
    """The normalised draw weights [E] (w / w.sum(); uniform for None) or a refusal that names the limit."""
    if draw_weights is None:
        w = np.ones(E)
    else:
        w = np.asarray(draw_weights, dtype=np.float64)
        if w.shape != (E,):
            raise ValueError(f"draw_weights must be [{E}] numbers, one per draw, got shape {list(w.shape)}")
        if not np.isfinite(w).all() or np.any(w < 0):
            raise ValueError("draw_weights must be non-negative finite numbers (a negative or non-finite weight is refused)")
        if not np.any(w > 0):
            raise ValueError("draw_weights are all zero: at least one draw must weigh something")
    return np.ascontiguousarray(w / w.sum())


def _prepare_control_pooled(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds, targets,
                            weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter, tol,
                            draw_weights, keep):
    p = _prepare_control(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds, targets,
                         weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter, tol, keep)
    p.update(pool_w=_pool_weights(draw_weights, p['E']), pool_given=draw_weights is not None)
    return p


def _trial_step(zi, g, trial):
    """slope [2, 31, n] = sum_d g_d (trial_d - z_d) in index order from 0.0, and moved [2, 31, n]: some trial_d != z_d.
    zi, g [D, n]; trial [D, 2, 31, n]."""
    slope, moved = np.zeros(trial.shape[1:]), np.zeros(trial.shape[1:], dtype=bool)
    with np.errstate(all='ignore'):
        step = trial - zi[:, np.newaxis, np.newaxis, :]
        for d in range(zi.shape[0]):
            slope = slope + g[d] * step[d]
            moved |= np.abs(step[d]) > 0
    return slope, moved


def _armijo(Ft, F, noise, slope, moved):
    """The Armijo decision of every solve: Ft, slope, moved [2, 31, n]; F, noise [n] -> (chosen [n], any_ok [n]).  chosen
    counts the 62 trials, the 31 Newton trials first; the first passing one is taken."""
    with np.errstate(all='ignore'):
        ok = moved & (Ft <= (F + ARMIJO * np.where(slope < 0, slope, 0.0)) + NOISE * noise)
    ok = ok.reshape(2 * CONTROL_TRIALS, -1)
    return np.argmax(ok, axis=0), ok.any(axis=0)


def _first_trial(S, E, D, idx, trial, slope, moved, Ft_draws, F, noise, g, **risk):
    """The trial half of iteration 0 for the starts idx that reached it, over all S starts (NaN, moved False elsewhere):
    trial [S, D, 2, 31], slope, moved [S, 2, 31], Ft_draws [S, E, 2, 31] (NaN for a draw of weight 0), F, noise [S] and g
    [S, D] as the decision reads them, the risk's own arrays [S, 2, 31] (``Ft``, or ``phi_t`` and ``a_t``), idle_moved [S, 2]
    (lanes 31 and 63 of the device's wavefront are no trials: 0), reached [S].  ``_first_trial_decision`` adds the rest."""
    n = idx.size
    full = lambda shape, values: _scatter(np.full((S,) + shape, np.nan), idx, values)
    out = dict(trial=full((D, 2, CONTROL_TRIALS), np.moveaxis(trial, -1, 0)), slope=full((2, CONTROL_TRIALS), np.moveaxis(slope, -1, 0)),
               moved=_scatter(np.zeros((S, 2, CONTROL_TRIALS), dtype=bool), idx, np.moveaxis(moved, -1, 0)),
               idle_moved=np.zeros((S, 2), dtype=np.int32),
               Ft_draws=full((E, 2, CONTROL_TRIALS), np.moveaxis(Ft_draws.reshape(E, 2, CONTROL_TRIALS, n), -1, 0)),
               F=full((), F), noise=full((), noise), g=full((D,), g.T), reached=_scatter(np.zeros(S, dtype=bool), idx, True))
    for key, value in risk.items():
        out[key] = full((2, CONTROL_TRIALS), np.moveaxis(value.reshape(2, CONTROL_TRIALS, n), -1, 0))
    return out


def _scatter(into, idx, values):
    into[idx] = values
    return into


def _first_trial_decision(first_trial, idx, chosen, any_ok, z, status, descent):
    """lane [S]: the trial taken, numbered as the device's wavefront lane (0-30 a Newton trial, 32-62 a steepest-descent
    trial), -1 where none passed or the start never got there; z [S, D], status (-1: the start goes on) and descent_steps
    [S] after iteration 0."""
    lane = np.full(status.shape[0], -1, dtype=np.int64)
    lane[idx] = np.where(any_ok, chosen + (chosen >= CONTROL_TRIALS), -1)
    first_trial.update(lane=lane, z=z.T.copy(), status=status.copy(), descent_steps=descent.copy())


def _control_pooled_solve_host(p):
    """Every start's pooled solve -> dict(z [S, D], cost, cost_start, status, iterations, descent_steps [S] and, with
    max_iter == 0, the first tangent pass: pooled F [S], g [S, D], H [S, D, D] and the draws' own F_draws [S, E], g_draws
    [S, E, D], H_draws [S, E, D, D]; NaN for a draw of weight 0, which is never evaluated).  Where iteration 0 reached its
    trial pass in some start, ``first_trial``: that pass (``_first_trial``, with the pooled ``Ft`` [S, 2, 31], and
    ``_first_trial_decision``)."""
    E, S, D, max_iter, tol, w = p['E'], p['starts'], p['D'], p['max_iter'], p['tol'], p['pool_w']
    live = np.flatnonzero(w != 0)
    z = np.array(p['z0'].T, order='C')                                # [D, S]; a copy: p['z0'] stays the start (for D == 1 .T is contiguous)
    status = np.full(S, -1, dtype=np.int32)
    iterations, descent = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    cost, cost_start = np.full(S, np.nan), np.full(S, np.nan)
    first_pass = first_trial = None

    def per_draw(values, n):
        """[..., live x n] as _control_pass returns it (draw-major) -> [E, ..., n], NaN where the draw weighs nothing"""
        out = np.full((E,) + values.shape[:-1] + (n,), np.nan)
        out[live] = np.moveaxis(values.reshape(values.shape[:-1] + (live.size, n)), -2, 0)
        return out

    for it in range(max_iter + 1):
        idx = np.flatnonzero(status < 0)
        n = idx.size
        if n == 0:
            break
        zi = z[:, idx]
        out = _control_pass(p, np.ascontiguousarray(np.tile(zi, (1, live.size))), np.repeat(live, n), tangents=True)
        parts = {key: per_draw(out[key], n) for key in ('F', 'noise', 'g', 'H')}
        F, noise, g, H = (pooled_sum(parts[key], w) for key in ('F', 'noise', 'g', 'H'))
        if it == 0:
            cost_start[idx] = F
            first_pass = dict(F=F.copy(), g=g.T.copy(), H=H.transpose(2, 0, 1).copy(), F_draws=parts['F'].T.copy(),
                              g_draws=parts['g'].transpose(2, 0, 1).copy(), H_draws=parts['H'].transpose(3, 0, 1, 2).copy())
        cost[idx] = F
        with np.errstate(all='ignore'):
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)
            pg = np.zeros(n)
            for d in range(D):
                pg = np.fmax(pg, np.abs(_clip01(zi[d] - g[d]) - zi[d]))
        code = np.where(~finite, NON_FINITE, np.where(pg <= tol, CONVERGED, ITERATION_LIMIT if it == max_iter else -1))
        stopped = code >= 0
        status[idx[stopped]], iterations[idx[stopped]] = code[stopped], it
        go = np.flatnonzero(~stopped)
        if go.size == 0:
            continue
        idx, zi, F, g, H, noise = idx[go], zi[:, go], F[go], g[:, go], H[:, :, go], noise[go]
        n = idx.size
        with np.errstate(all='ignore'):
            active = ((zi <= 0.0) & (g > 0)) | ((zi >= 1.0) & (g < 0))
            direction = _control_direction(H, g, active)
            both = np.stack([direction, -g], axis=1)                                              # [D, 2, n]
            trial = _clip01(zi[:, np.newaxis, np.newaxis, :] + _TRIAL_ALPHA[np.newaxis, np.newaxis, :, np.newaxis] *
                            both[:, :, np.newaxis, :])                                            # [D, 2, 31, n]
            m = 2 * CONTROL_TRIALS * n
            flat = trial.reshape(D, m)
            Ft_draws = per_draw(_control_pass(p, np.ascontiguousarray(np.tile(flat, (1, live.size))), np.repeat(live, m))['F'], m)
            Ft = pooled_sum(Ft_draws, w).reshape(2, CONTROL_TRIALS, n)
            slope, moved = _trial_step(zi, g, trial)
        chosen, any_ok = _armijo(Ft, F, noise, slope, moved)          # the first Newton lane, else the first steepest-descent lane
        taken = trial.reshape(D, 2 * CONTROL_TRIALS, n)[:, chosen, np.arange(n)]
        z[:, idx[any_ok]] = taken[:, any_ok]
        descent[idx[any_ok & (chosen >= CONTROL_TRIALS)]] += 1
        status[idx[~any_ok]], iterations[idx[~any_ok]] = STALLED, it
        if it == 0:
            first_trial = _first_trial(S, E, D, idx, trial, slope, moved, Ft_draws, F, noise, g, Ft=Ft)
            _first_trial_decision(first_trial, idx, chosen, any_ok, z, status, descent)
    res = dict(z=z.T.copy(), cost=cost, cost_start=cost_start, status=status, iterations=iterations, descent_steps=descent)
    if max_iter == 0:
        res['first_pass'] = first_pass
    if first_trial is not None:
        res['first_trial'] = first_trial
    return res


def _run_control_pooled_host(p):
    solved = _control_pooled_solve_host(p)
    best = int(_best_start(solved['cost'][np.newaxis], solved['status'][np.newaxis])[0])
    zb = np.ascontiguousarray(np.repeat(solved['z'][best][:, np.newaxis], p['E'], axis=1))
    out = _control_pass(p, zb, np.arange(p['E']), record=True)
    return solved, best, out['members'], out['first'], out['F']


def _weighted_band(values, w):
    """The weighted 2.5 % / 97.5 % quantiles of values [E, ...] over the draws, by ``_assemble_assimilate``'s rule."""
    live = np.flatnonzero(w > 0)
    flat = values[live].reshape(live.size, -1)
    band = np.empty((flat.shape[1], 2))
    for k in range(flat.shape[1]):
        order = np.argsort(flat[:, k], kind='stable')
        cumulative = np.cumsum(w[live][order])
        cumulative = cumulative / cumulative[-1]
        for side, level in enumerate((0.025, 0.975)):
            band[k, side] = flat[order[min(int(np.searchsorted(cumulative, level)), live.size - 1)], k]
    return band.reshape(values.shape[1:] + (2,))


def _assemble_control_pooled(p, solved, best, members, first, cost_draws):
    E, nc, Kseg, w = p['E'], p['n_controls'], p['segments'], p['pool_w']
    true_scale = lambda zz: p['ctl_lo'][:, np.newaxis] + zz.reshape(zz.shape[:-1] + (nc, Kseg)) * p['ctl_width'][:, np.newaxis]
    z = solved['z'][best]
    u = true_scale(z)
    with np.errstate(all='ignore'):
        outside = (members > p['lim_hi'][np.newaxis, :, np.newaxis]) | (members < p['lim_lo'][np.newaxis, :, np.newaxis])
    violated = outside[:, :, 1:].any(axis=2)                          # the points the cost sees: 1 .. P - 1
    res = SimulateResult(u=u, z=z.reshape(nc, Kseg), cost=float(solved['cost'][best]), status=int(solved['status'][best]),
                         iterations=int(solved['iterations'][best]), descent_steps=int(solved['descent_steps'][best]),
                         cost_start=float(solved['cost_start'][best]), best_start=int(best), u_mean=u, cost_draws=cost_draws,
                         draw_weights=w, t=p['T'], mean=pooled_sum(members, w), first_saturation=first, violated=violated,
                         violation_share=pooled_sum(violated.astype(np.float64), w), controls=list(p['controls']),
                         states=list(p['states']), segment_first=p['seg_first'].astype(np.int64), pooled=True)
    if p['pool_given']:
        res['bounds'] = _weighted_band(members, w)
    elif E >= 2:
        cut = bounds_cut(E)
        ms = np.sort(members, axis=0)
        res['bounds'] = np.stack([ms[cut], ms[E - cut]], axis=-1)
    if p['want_members']:
        res['members'] = members
    if p['want_all']:
        res.update(u_all=true_scale(solved['z']), cost_all=solved['cost'], status_all=solved['status'],
                   iterations_all=solved['iterations'], descent_steps_all=solved['descent_steps'])
    if 'first_pass' in solved:
        res['first_pass'] = solved['first_pass']
    return res


_CONTROL_POOLED_SIGNATURE = """
    Every argument shared with ``control`` means what it means there (its docstring).
    draw_weights : None (uniform) or [E] non-negative numbers, for example ``assimilate``'s ``weights``; normalised as
                  w / w.sum().  A draw of weight 0 is never evaluated by the solver.  A wrong length, a negative or non-finite
                  weight and all weights zero are refused
    starts      : ``control``'s starts; there are ``starts`` solves in all
    max_iter=0  : returns ``first_pass``: the pooled F [S], g [S, D], H [S, D, D] and the draws' own F_draws [S, E], g_draws
                  [S, E, D], H_draws [S, E, D, D] (NaN for a draw of weight 0)

    Returns a ``SimulateResult``: of the best start u [n_controls, K] (true scale), z, cost, cost_start, status, iterations,
    descent_steps and best_start (scalars; the best start has the smallest finite cost); u_mean = u, so
    ``expand_controls(res)`` gives the ``forcing`` arrays (``expand_controls(res, e)`` is refused: there is no per-draw
    sequence); cost_draws [E], every draw's own cost F_e at u; draw_weights [E] as normalised; t, first_saturation [E] and
    with keep='members' members [E, n_states, P]: every draw's trajectory under the shared u; mean [n_states, P] =
    ``pooled_sum(members, w)``; bounds [n_states, P, 2]: ``evaluate``'s order statistics for uniform weights (E >= 2), else
    the weighted 2.5 % / 97.5 % quantiles over the draws of positive weight; violated [E, n_states] bool: some point 1 .. P - 1
    of the trajectory lies outside ``limits``; violation_share [n_states]: the weight of those draws; u_all, cost_all,
    status_all, iterations_all, descent_steps_all [S, ...] with keep='all'."""


def control_pooled(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None, segments=8,
                   control_bounds=None, targets=None, weights=None, terminal=None, limits=None, limit_weight=1e3,
                   move_weight=None, previous=None, init=None, starts=1, max_iter=60, tol=1e-10, draw_weights=None, keep=None,
                   device=None):
    """One control sequence for the whole posterior: the expected cost sum_e w_e F_e(z) of ``control``'s cost over the draws,
    minimised over one decision vector, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_control_pooled(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds,
                                targets, weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter,
                                tol, draw_weights, keep)
    ctx = _device_context(device)
    return _assemble_control_pooled(p, *ctx.control_pooled_solve(p))


def control_pooled_host(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None,
                        segments=8, control_bounds=None, targets=None, weights=None, terminal=None, limits=None,
                        limit_weight=1e3, move_weight=None, previous=None, init=None, starts=1, max_iter=60, tol=1e-10,
                        draw_weights=None, keep=None):
    """``control_pooled`` in numpy on this host, vectorised over starts, draws and trial points: the statement the kernels are
    tested against (module docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare_control_pooled(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds,
                                targets, weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter,
                                tol, draw_weights, keep)
    return _assemble_control_pooled(p, *_run_control_pooled_host(p))


control_pooled.__doc__ += _CONTROL_POOLED_SIGNATURE
control_pooled_host.__doc__ += _CONTROL_POOLED_SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# control_cvar: one control sequence that protects the bad tail of the posterior (module docstring)
# ---------------------------------------------------------------------------------------------------------

CVAR_BISECTIONS = 64


def cvar_exact(F, w, alpha):
    """The exact CVaR at level alpha of the costs F [E] under the weights w [E], and the VaR -> (cvar, var).  The live
    draws (w_e != 0) are ranked by F descending, ties to the lower index; the mass is accumulated sequentially in that
    order; a draw strictly inside the mass m = 1 - alpha counts fully, the boundary draw (its cost is the VaR) gets m minus
    the mass before it; the sum is divided by m.  A non-finite live cost gives (NaN, NaN)."""
    F, w, m = np.asarray(F, dtype=np.float64), np.asarray(w, dtype=np.float64), 1.0 - float(alpha)
    if F.ndim != 1 or F.shape != w.shape:
        raise ValueError(f"cvar_exact: F and w must be [E] numbers, got shapes {list(F.shape)} and {list(w.shape)}")
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError(f"alpha must lie in [0, 1), got {alpha}")
    live = np.flatnonzero(w != 0)
    if live.size == 0 or not np.isfinite(F[live]).all():
        return np.nan, np.nan
    order = live[np.argsort(-F[live], kind='stable')]
    before, total, var = 0.0, 0.0, F[order[-1]]
    for e in order:
        if before + w[e] < m:
            total = total + w[e] * F[e]
            before = before + w[e]
        else:
            total = total + (m - before) * F[e]
            var = F[e]
            break
    return float(total / m), float(var)


def _smooth_plus(t, eps):
    """s_eps(t): 0 for t <= 0, t^2 / (2 eps) for 0 < t < eps, t - eps / 2 from eps on (C1)"""
    return np.where(t <= 0.0, 0.0, np.where(t < eps, (t * t) / (2.0 * eps), t - 0.5 * eps))


def cvar_smooth(F, w, alpha, eps):
    """The smoothed Rockafellar-Uryasev risk of the costs F [E, ...] under the weights w [E] (every trailing index is a
    risk of its own) -> (phi [...], a [...], q [E, ...], c [E, ...]):

        phi = min_a  a + (1 / m) sum_e w_e s_eps(F_e - a),   m = 1 - alpha

    ``a`` by ``CVAR_BISECTIONS`` = 64 bisections of h(a) = pooled_sum(clip((F - a) / eps, 0, 1), w) = m from
    [min F - eps, max F] over the live draws (mid = lo + 0.5 (hi - lo); lo = mid if h > m, else hi = mid; a = hi);
    r = clip((F - a) / eps, 0, 1), the soft tail weights q_e = (w_e r_e) / m and the band weights c_e = w_e / (m eps) where
    0 < F_e - a < eps (else 0).  A draw of weight 0 has q = c = 0 and may hold anything.  A non-finite live cost gives
    phi = a = NaN and q = c = 0.  Only + - * /, comparisons and ``pooled_sum``."""
    F, w = np.asarray(F, dtype=np.float64), np.asarray(w, dtype=np.float64)
    m, eps = 1.0 - float(alpha), float(eps)
    if w.ndim != 1 or F.ndim < 1 or F.shape[0] != w.shape[0]:
        raise ValueError(f"cvar_smooth: F must hold one row per weight ({list(w.shape)}), got shape {list(F.shape)}")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"cvar_smooth: alpha must lie in (0, 1), got {alpha} (alpha = 0 is the plain pooled sum)")
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"epsilon must be positive and finite, got {eps}")
    live = w != 0
    if not live.any():
        raise ValueError("cvar_smooth: the weights are all zero")
    wide = live.reshape((-1,) + (1,) * (F.ndim - 1))
    with np.errstate(all='ignore'):
        bad = (wide & ~np.isfinite(F)).any(axis=0)
        Fs = np.where(wide & ~bad, F, 0.0)                             # what is not live, or sits in a non-finite risk: 0
        lo = np.min(np.where(wide, Fs, np.inf), axis=0) - eps
        hi = np.max(np.where(wide, Fs, -np.inf), axis=0)
        for _ in range(CVAR_BISECTIONS):
            mid = lo + 0.5 * (hi - lo)
            above = pooled_sum(_clip01((Fs - mid) / eps), w) > m
            lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
        a = hi
        t = Fs - a
        q = np.where(wide & ~bad, (w.reshape(wide.shape) * _clip01(t / eps)) / m, 0.0)
        c = np.where(wide & ~bad & (t > 0.0) & (t < eps), w.reshape(wide.shape) / (m * eps), 0.0) + np.zeros_like(Fs)
        phi = a + pooled_sum(_smooth_plus(t, eps), w) / m
    return np.where(bad, np.nan, phi), np.where(bad, np.nan, a), q, c


def _pooled_sum_each(X, q):
    """``pooled_sum`` with weights of their own per last index: X [E, ..., n], q [E, n] -> [..., n]; where q[e, k] == 0 the
    draw is skipped for index k (its X may hold anything)."""
    total = None
    with np.errstate(all='ignore'):
        for begin in range(0, q.shape[0], POOL_CHUNK):
            acc = np.zeros(X.shape[1:])
            for e in range(begin, min(begin + POOL_CHUNK, q.shape[0])):
                acc = np.where(q[e] != 0, acc + q[e] * X[e], acc)
            total = acc if total is None else total + acc
    return total


def _cvar_pooled(parts, w, alpha, eps):
    """phi, noise, g, H of one tangent pass from the draws' own parts (F, noise [E, n], g [E, D, n], H [E, D, D, n]), and
    a, q, c (module docstring: the pooled quantities)."""
    phi, a, q, c = cvar_smooth(parts['F'], w, alpha, eps)
    noise, g, Hq = (_pooled_sum_each(parts[key], q) for key in ('noise', 'g', 'H'))
    ge = parts['g']
    with np.errstate(all='ignore'):
        sc = _pooled_sum_each(np.ones_like(parts['F']), c)
        scg = _pooled_sum_each(ge, c)
        scgg = _pooled_sum_each(ge[:, :, np.newaxis, :] * ge[:, np.newaxis, :, :], c)
        bracket = scgg - (scg[:, np.newaxis, :] * scg[np.newaxis, :, :]) / sc
        H = np.where(sc != 0, Hq + bracket, Hq)
    return phi, noise, g, H, a, q, c


def _check_cvar(alpha, smoothing, epsilon):
    alpha = float(alpha)
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"alpha must lie in [0, 1), got {alpha}")
    smoothing = float(smoothing)
    if not (smoothing > 0 and np.isfinite(smoothing)):
        raise ValueError(f"smoothing must be positive and finite, got {smoothing}")
    if epsilon is not None:
        epsilon = float(epsilon)
        if not (epsilon > 0 and np.isfinite(epsilon)):
            raise ValueError(f"epsilon must be positive and finite, got {epsilon}")
    return alpha, smoothing, epsilon


def _relative_epsilon(smoothing, cost):
    """eps = smoothing x the pooled cost of start 0 at its z0, or the refusal"""
    if not (np.isfinite(cost) and cost != 0):
        raise ValueError(f"smoothing is relative to the pooled cost at the start, which is {cost}: with a cost of 0 or a "
                         "non-finite cost there give epsilon= in cost units")
    return float(smoothing * cost)


def _control_cvar_solve_host(p):
    """Every start's CVaR solve -> ``_control_pooled_solve_host``'s dict with cost = phi, ``epsilon`` and, with
    max_iter == 0, the first pass: phi, a [S], g [S, D], H [S, D, D], q, c [S, E] and the draws' own parts; ``first_trial``
    holds ``phi_t`` and ``a_t`` [S, 2, 31] (``cvar_smooth`` of every trial point's costs) in place of the pooled ``Ft``, and
    F is phi."""
    E, S, D, max_iter, tol, w = p['E'], p['starts'], p['D'], p['max_iter'], p['tol'], p['pool_w']
    alpha, eps = p['alpha'], p['epsilon']
    live = np.flatnonzero(w != 0)
    z = np.array(p['z0'].T, order='C')                                # [D, S]; a copy: p['z0'] stays the start (for D == 1 .T is contiguous)
    status = np.full(S, -1, dtype=np.int32)
    iterations, descent = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    cost, cost_start = np.full(S, np.nan), np.full(S, np.nan)
    first_pass = first_trial = None

    def per_draw(values, n):
        out = np.full((E,) + values.shape[:-1] + (n,), np.nan)
        out[live] = np.moveaxis(values.reshape(values.shape[:-1] + (live.size, n)), -2, 0)
        return out

    for it in range(max_iter + 1):
        idx = np.flatnonzero(status < 0)
        n = idx.size
        if n == 0:
            break
        zi = z[:, idx]
        out = _control_pass(p, np.ascontiguousarray(np.tile(zi, (1, live.size))), np.repeat(live, n), tangents=True)
        parts = {key: per_draw(out[key], n) for key in ('F', 'noise', 'g', 'H')}
        if it == 0 and eps is None:
            eps = _relative_epsilon(p['smoothing'], float(pooled_sum(parts['F'][:, 0], w)))
        F, noise, g, H, a, q, c = _cvar_pooled(parts, w, alpha, eps)
        if it == 0:
            cost_start[idx] = F
            first_pass = dict(phi=F.copy(), a=a.copy(), g=g.T.copy(), H=H.transpose(2, 0, 1).copy(), q=q.T.copy(), c=c.T.copy(),
                              F_draws=parts['F'].T.copy(), g_draws=parts['g'].transpose(2, 0, 1).copy(),
                              H_draws=parts['H'].transpose(3, 0, 1, 2).copy())
        cost[idx] = F
        with np.errstate(all='ignore'):
            finite = np.isfinite(F) & np.isfinite(g).all(axis=0)
            pg = np.zeros(n)
            for d in range(D):
                pg = np.fmax(pg, np.abs(_clip01(zi[d] - g[d]) - zi[d]))
        code = np.where(~finite, NON_FINITE, np.where(pg <= tol, CONVERGED, ITERATION_LIMIT if it == max_iter else -1))
        stopped = code >= 0
        status[idx[stopped]], iterations[idx[stopped]] = code[stopped], it
        go = np.flatnonzero(~stopped)
        if go.size == 0:
            continue
        idx, zi, F, g, H, noise = idx[go], zi[:, go], F[go], g[:, go], H[:, :, go], noise[go]
        n = idx.size
        with np.errstate(all='ignore'):
            active = ((zi <= 0.0) & (g > 0)) | ((zi >= 1.0) & (g < 0))
            direction = _control_direction(H, g, active)
            both = np.stack([direction, -g], axis=1)                                              # [D, 2, n]
            trial = _clip01(zi[:, np.newaxis, np.newaxis, :] + _TRIAL_ALPHA[np.newaxis, np.newaxis, :, np.newaxis] *
                            both[:, :, np.newaxis, :])                                            # [D, 2, 31, n]
            m = 2 * CONTROL_TRIALS * n
            flat = trial.reshape(D, m)
            Ft_draws = per_draw(_control_pass(p, np.ascontiguousarray(np.tile(flat, (1, live.size))), np.repeat(live, m))['F'], m)
            Ft, a_t = (x.reshape(2, CONTROL_TRIALS, n) for x in cvar_smooth(Ft_draws, w, alpha, eps)[:2])   # phi of every trial lane
            slope, moved = _trial_step(zi, g, trial)
        chosen, any_ok = _armijo(Ft, F, noise, slope, moved)
        taken = trial.reshape(D, 2 * CONTROL_TRIALS, n)[:, chosen, np.arange(n)]
        z[:, idx[any_ok]] = taken[:, any_ok]
        descent[idx[any_ok & (chosen >= CONTROL_TRIALS)]] += 1
        status[idx[~any_ok]], iterations[idx[~any_ok]] = STALLED, it
        if it == 0:
            first_trial = _first_trial(S, E, D, idx, trial, slope, moved, Ft_draws, F, noise, g, phi_t=Ft, a_t=a_t)
            _first_trial_decision(first_trial, idx, chosen, any_ok, z, status, descent)
    res = dict(z=z.T.copy(), cost=cost, cost_start=cost_start, status=status, iterations=iterations, descent_steps=descent,
               epsilon=eps)
    if max_iter == 0:
        res['first_pass'] = first_pass
    if first_trial is not None:
        res['first_trial'] = first_trial
    return res


def _run_control_cvar_host(p):
    if p['alpha'] == 0:
        return _run_control_pooled_host(p)
    solved = _control_cvar_solve_host(p)
    best = int(_best_start(solved['cost'][np.newaxis], solved['status'][np.newaxis])[0])
    zb = np.ascontiguousarray(np.repeat(solved['z'][best][:, np.newaxis], p['E'], axis=1))
    out = _control_pass(p, zb, np.arange(p['E']), record=True)
    return solved, best, out['members'], out['first'], out['F']


def _assemble_control_cvar(p, solved, best, members, first, cost_draws):
    res = _assemble_control_pooled(p, solved, best, members, first, cost_draws)
    w, alpha = p['pool_w'], p['alpha']
    cvar, var = cvar_exact(cost_draws, w, alpha)
    if alpha == 0:
        eps, a, q = (np.nan if p['epsilon'] is None else p['epsilon']), np.nan, w.copy()
    else:
        eps = float(solved['epsilon'])
        _, a, q, _ = cvar_smooth(cost_draws, w, alpha, eps)
        a = float(a)
    res.update(cvar=cvar, var=var, expected_cost=float(pooled_sum(cost_draws, w)), tail_weights=q, a=a, epsilon=eps, alpha=alpha)
    return res


_CONTROL_CVAR_SIGNATURE = """
    Every argument shared with ``control_pooled`` means what it means there (its docstring).
    alpha       : the level in [0, 1): the plan minimises the mean cost of the worst 1 - alpha of the posterior's weight.
                  alpha = 0 IS ``control_pooled``, bit for bit in every field
    smoothing   : epsilon=None takes eps = smoothing x the pooled cost of start 0 at its starting point (refused where that
                  cost is 0 or not finite); eps is fixed for the whole call and all starts
    epsilon     : the width of the smoothed kink in cost units, instead of ``smoothing``
    max_iter=0  : returns ``first_pass``: phi, a [S], g [S, D], H [S, D, D], q, c [S, E] and the draws' own F_draws [S, E],
                  g_draws [S, E, D], H_draws [S, E, D, D] (NaN for a draw of weight 0); for alpha = 0 ``control_pooled``'s

    Returns ``control_pooled``'s ``SimulateResult`` with cost = phi at the plan (cvar - eps / (2 (1 - alpha)) <= phi <= cvar)
    and cvar, var: the exact CVaR and VaR of cost_draws (``cvar_exact``); expected_cost = ``pooled_sum(cost_draws, w)``;
    tail_weights [E]: q at the plan; a; epsilon (NaN for alpha = 0 without ``epsilon=``); alpha."""


def control_cvar(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None, segments=8,
                 control_bounds=None, targets=None, weights=None, terminal=None, limits=None, limit_weight=1e3,
                 move_weight=None, previous=None, init=None, starts=1, max_iter=60, tol=1e-10, draw_weights=None, alpha=0.9,
                 smoothing=0.01, epsilon=None, keep=None, device=None):
    """One control sequence for the whole posterior that protects its bad tail: the smoothed conditional value at risk at
    level alpha of ``control``'s cost over the draws, minimised over one decision vector, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    alpha, smoothing, epsilon = _check_cvar(alpha, smoothing, epsilon)
    p = _prepare_control_pooled(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds,
                                targets, weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter,
                                tol, draw_weights, keep)
    p.update(alpha=alpha, smoothing=smoothing, epsilon=epsilon)
    ctx = _device_context(device)
    return _assemble_control_cvar(p, *ctx.control_cvar_solve(p))


def control_cvar_host(models, states, inputs, controls=None, forcing=None, y0=None, t=None, draws=None, bounds=None,
                      segments=8, control_bounds=None, targets=None, weights=None, terminal=None, limits=None,
                      limit_weight=1e3, move_weight=None, previous=None, init=None, starts=1, max_iter=60, tol=1e-10,
                      draw_weights=None, alpha=0.9, smoothing=0.01, epsilon=None, keep=None):
    """``control_cvar`` in numpy on this host: the statement the kernels are tested against (module docstring), not a
    fallback.  Same arguments, same result fields."""
    alpha, smoothing, epsilon = _check_cvar(alpha, smoothing, epsilon)
    p = _prepare_control_pooled(models, states, inputs, controls, forcing, y0, t, draws, bounds, segments, control_bounds,
                                targets, weights, terminal, limits, limit_weight, move_weight, previous, init, starts, max_iter,
                                tol, draw_weights, keep)
    p.update(alpha=alpha, smoothing=smoothing, epsilon=epsilon)
    return _assemble_control_cvar(p, *_run_control_cvar_host(p))


control_cvar.__doc__ += _CONTROL_CVAR_SIGNATURE
control_cvar_host.__doc__ += _CONTROL_CVAR_SIGNATURE


# ---------------------------------------------------------------------------------------------------------
# calibrate: an ensemble sampler over initial states and constant parameters, per posterior draw (module docstring)
# ---------------------------------------------------------------------------------------------------------

WALKERS = _capi.CALIBRATE_WALKERS
HALF_WALKERS = WALKERS // 2
MAX_UNKNOWN = _capi.CALIBRATE_MAX_UNKNOWN
JITTER = 1e-5
_KEEP_CALIBRATE = ('x', 'trajectories')


def calibrate_lds_bytes(n_factors, n_norm_state, n_coef, d):
    """LDS bytes of a draw's wavefront: slot 0, the factors and the normalised states as [item][lane], 7 d rows (both
    halves' positions, the proposal, two halves x (sum, sum of squares)), and the draw's coefficients once."""
    return (1 + n_factors + n_norm_state + 7 * d) * LANES * 8 + n_coef * 8


def _prepare_calibrate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, unknown=None, observe=None,
                       data=None, obs_points=None, every=None, obs_sd=None, prior=None, unknown_bounds=None, starts=None,
                       burnin=300, draws_kept=200, thin=10, jump_every=8, seed=0, keep='x'):
    """``_prepare`` with the parameters as placeholder forcing columns, and what the sampler adds; touches no device."""
    wanted = {keep} if isinstance(keep, str) else set(keep or ())
    if not wanted <= set(_KEEP_CALIBRATE):
        raise ValueError("keep must be None, 'x', 'trajectories' or a list of the two")
    if unknown is None or isinstance(unknown, str):
        unknown = [unknown] if unknown is not None else []
    unknown = [str(name) for name in unknown]
    d = len(unknown)
    if d < 1 or d > MAX_UNKNOWN:
        raise ValueError(f"unknown must list 1 to {MAX_UNKNOWN} unknowns ('y0:<state>' or a parameter's name), got {d}")
    for name in unknown:
        if unknown.count(name) > 1:
            raise ValueError(f"unknown names '{name}' twice")
    forcing = {str(key): values for key, values in dict(forcing or {}).items()}
    state_names = [str(name) for name in states]
    parameters = []
    for name in unknown:
        if name.startswith('y0:'):
            if name[3:] not in state_names:
                raise ValueError(f"unknown: '{name}' names no state ({state_names})")
            continue
        if name in state_names:
            raise ValueError(f"unknown: '{name}' is a state (its initial value is 'y0:{name}')")
        if name in forcing:
            raise ValueError(f"unknown: '{name}' is a forcing key")
        parameters.append(name)
    start, stop, h = (float(v) for v in t)
    if not (np.isfinite([start, stop, h]).all() and h > 0):
        raise ValueError("t = (start, stop, h) needs finite numbers and h > 0")
    n_steps = max(len(np.arange(start, stop + h, h)) - 1, 0)
    placeholder = np.zeros(n_steps)
    p = _prepare(models, states, inputs, {**forcing, **{name: placeholder for name in parameters}}, y0, t, draws, bounds, False,
                 None, lds_per_member=False)
    K, E, P = p['K'], p['E'], p['n_steps'] + 1
    states = p['states']
    names, points, data, obs_sd = _prepare_observations(states, P, observe, data, obs_points, every, obs_sd)

    # ---- the unknowns: their sources and the open box ----
    unknown_src = np.empty(d, dtype=np.int32)
    for i, name in enumerate(unknown):
        if name.startswith('y0:'):
            unknown_src[i] = states.index(name[3:])
        else:
            if name not in p['forcing_cols']:
                raise ValueError(f"unknown: no model reads '{name}' (no term of any model has an order on it)")
            unknown_src[i] = -(p['forcing_cols'].index(name) + 1)
    norm_param = np.full(p['n_norm_forcing'], -1, dtype=np.int32)
    for n in range(p['n_norm_forcing']):
        hit = np.flatnonzero(unknown_src == p['norm_src'][n])
        if hit.size:
            norm_param[n] = hit[0]
    given = {str(key): value for key, value in dict(unknown_bounds or {}).items()}
    for name in given:
        if name not in unknown:
            raise ValueError(f"unknown_bounds: '{name}' is not an unknown ({unknown})")
    lo, hi = np.empty(d), np.empty(d)
    for i, name in enumerate(unknown):
        if unknown_src[i] < 0:
            lo[i], hi[i] = _column_box(p, np.flatnonzero(norm_param == i), name, given, 'unknown_bounds', 'parameter')
            continue
        box_lo, box_hi = p['box'][unknown_src[i]]
        if name in given:
            pair = np.asarray(given[name], dtype=np.float64)
            if pair.shape != (2,) or not np.isfinite(pair).all():
                raise ValueError(f"unknown_bounds['{name}'] must be two finite numbers (lo, hi) in true scale")
            lo[i], hi[i] = pair
            if not lo[i] < hi[i]:
                raise ValueError(f"unknown_bounds['{name}'] is empty (lower {lo[i]}, upper {hi[i]})")
            if lo[i] < box_lo or hi[i] > box_hi:
                raise ValueError(f"unknown_bounds['{name}'] reaches outside the box [{box_lo}, {box_hi}] of the state")
        else:
            lo[i], hi[i] = box_lo, box_hi
        if not np.isfinite([lo[i], hi[i]]).all():
            raise ValueError(f"unknown '{name}': its box [{lo[i]}, {hi[i]}] is not finite (no model reads the state): give "
                             f"bounds or unknown_bounds")

    # ---- the prior, the starts, the sampler's settings ----
    prior_mean, prior_prec = np.zeros(d), np.zeros(d)
    for key, pair in dict(prior or {}).items():
        if str(key) not in unknown:
            raise ValueError(f"prior: '{key}' is not an unknown ({unknown})")
        if np.ndim(pair) != 1 or len(pair) != 2:
            raise ValueError(f"prior['{key}'] must be (mean, sd) with a finite mean and sd > 0 (true scale)")
        mu, sd = float(pair[0]), float(pair[1])
        if not (np.isfinite(mu) and sd > 0 and np.isfinite(sd)):
            raise ValueError(f"prior['{key}'] must be (mean, sd) with a finite mean and sd > 0 (true scale)")
        i = unknown.index(str(key))
        prior_mean[i], prior_prec[i] = mu, 1.0 / (sd * sd)
    if starts is None:
        x0 = start_points(WALKERS, lo, hi)
    else:
        x0 = np.array(starts, dtype=np.float64)
        if x0.shape != (WALKERS, d) or not np.isfinite(x0).all():
            raise ValueError(f"starts must be finite numbers [{WALKERS}, {d}] (true scale)")
    if not np.all((x0 > lo) & (x0 < hi)):
        raise ValueError("every start must lie strictly inside the box")
    for name, value, least in (('burnin', burnin, 0), ('draws_kept', draws_kept, 1), ('thin', thin, 1),
                               ('jump_every', jump_every, 0)):
        if isinstance(value, str) or np.ndim(value) != 0 or int(value) != value or int(value) < least:
            raise ValueError(f"{name} must be an integer >= {least}")
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    n_factors, n_norm_state, n_coef = p['fac_norm'].shape[0], p['norm_src'].shape[0] - p['n_norm_forcing'], p['coef'].shape[0]
    lds_bytes = calibrate_lds_bytes(n_factors, n_norm_state, n_coef, d)
    if lds_bytes > LDS_BUDGET:
        raise ValueError(f"the problem needs {lds_bytes} bytes of LDS ((1 + {n_factors} factors + {n_norm_state} normalised "
                         f"states + 7 x {d} unknowns) x {LANES} x 8 + {n_coef} coefficients x 8), a wavefront has {LDS_BUDGET}")
    obs_row = np.full(P, -1, dtype=np.int32)
    obs_row[points] = np.arange(points.shape[0], dtype=np.int32)
    n_rows = np.atleast_2d(np.asarray(_model_fields(models[0], 0)['betas'])).shape[0]
    p.update(d=d, unknown=unknown, unknown_src=unknown_src, norm_param=norm_param, lo=lo, hi=hi, prior_mean=prior_mean,
             prior_prec=prior_prec, starts=np.ascontiguousarray(x0), obs_names=names,
             obs_state=np.array([states.index(name) for name in names], dtype=np.int32), obs_sd=obs_sd,
             obs_hp=0.5 / (obs_sd * obs_sd), obs_points=points.astype(np.int64), obs_row=obs_row,
             data=np.ascontiguousarray(data), burnin=int(burnin), draws_kept=int(draws_kept), thin=int(thin),
             jump_every=int(jump_every), seed=int(seed) & 0xFFFFFFFF, draw_ids=_draw_ids(n_rows, draws, E),
             want_rows='x' in wanted, want_trajectories='trajectories' in wanted, lds_bytes=lds_bytes)
    return p


def calibrate_target(p, theta, trajectories=False):
    """lp [E, n] and saturated [E, n] at theta [E, n, d] (true scale, inside the box): the module docstring's trajectory and
    sums in its order, vectorised over (draw, walker).  ``trajectories``: also the points [E, n, K, P]."""
    K, E, S, n, d = p['K'], p['E'], p['n_steps'], theta.shape[1], p['d']
    M = E * n
    wide = dict(p, coef=np.repeat(p['coef'], n, axis=1))              # member e * n + i is walker i of draw e
    th = np.ascontiguousarray(theta.reshape(M, d).T)
    y = np.repeat(p['y0'], n, axis=1)
    for i in range(d):
        if p['unknown_src'][i] >= 0:
            y[p['unknown_src'][i]] = th[i]
    fac = np.ones((1 + p['fac_norm'].shape[0], M))
    xn = np.zeros((p['norm_src'].shape[0], M))
    acted = np.zeros(M, dtype=bool)
    constant = [f for f in range(p['n_forcing_factors']) if p['norm_param'][p['fac_norm'][f]] >= 0]
    stepwise = [f for f in range(p['n_forcing_factors']) if p['norm_param'][p['fac_norm'][f]] < 0]
    for f in constant:                                                # once per trajectory
        m = p['fac_norm'][f]
        xn[m], clamp = _clamped((th[p['norm_param'][m]] - p['norm_lo'][m]) / p['norm_span'][m])
        acted |= clamp
        _factor_values(p, fac, xn, f, f + 1)
    points = np.empty((K, S + 1, M)) if trajectories else None
    ss = np.zeros(M)

    def observe(point, ss):
        r = p['obs_row'][point]
        if r < 0:
            return ss
        for o in range(p['obs_state'].shape[0]):
            if not np.isnan(p['data'][r, o]):
                res = p['data'][r, o] - y[p['obs_state'][o]]
                ss = ss + p['obs_hp'][o] * (res * res)
        return ss

    if trajectories:
        points[:, 0] = y
    ss = observe(0, ss)
    for s in range(S):
        for f in stepwise:                                            # once per step
            m = p['fac_norm'][f]
            x = np.full(M, p['forcing'][s, -(p['norm_src'][m] + 1)])
            xn[m], clamp = _clamped((x - p['norm_lo'][m]) / p['norm_span'][m])
            acted |= clamp
            _factor_values(p, fac, xn, f, f + 1)
        y, stages_acted = _stages(wide, fac, xn, y)
        acted |= stages_acted
        if trajectories:
            points[:, s + 1] = y
        ss = observe(s + 1, ss)
    pp = np.zeros(M)
    for i in range(d):
        dl = th[i] - p['prior_mean'][i]
        pp = pp + p['prior_prec'][i] * (dl * dl)
    lp = (-ss - 0.5 * pp).reshape(E, n)
    if trajectories:
        return lp, acted.reshape(E, n), np.ascontiguousarray(points.reshape(K, S + 1, E, n).transpose(2, 3, 0, 1))
    return lp, acted.reshape(E, n)


def _run_calibrate_host(p):
    """-> (x [E, kept, 128, d], lp [E, kept, 128], saturated [E, kept, 128] (the three None without rows), sums [E, 128, 2, 2,
    d], accepted [E, 128, 2], evaluations [E], invalid [E], trajectories [E, 128, K, P] or None): what
    ``DeviceContext.calibrate`` returns."""
    E, d, W, H = p['E'], p['d'], WALKERS, HALF_WALKERS
    lo, hi, ids, seed, thin, rows = p['lo'], p['hi'], p['draw_ids'], p['seed'], p['thin'], p['want_rows']
    burnin, draws, jump_every = p['burnin'], p['draws_kept'], p['jump_every']
    x = np.broadcast_to(p['starts'], (E, W, d)).copy()
    with np.errstate(all='ignore'):
        lp, sat = calibrate_target(p, x)
    invalid = ~np.isfinite(lp).all(axis=1)
    iterations, first_half, kept = burnin + draws, draws // 2, -(-draws // thin)
    x_rows = np.empty((E, kept, W, d)) if rows else None
    lp_rows = np.empty((E, kept, W)) if rows else None
    sat_rows = np.empty((E, kept, W), dtype=bool) if rows else None
    sums = np.zeros((E, W, 2, 2, d))
    acc = np.zeros((E, W, 2, d))
    accepted = np.zeros((E, W, 2), dtype=np.int32)
    evaluations = np.full(E, W, dtype=np.int64)
    shift = 0.5 * (lo + hi)
    rng = lambda t, purpose, count: _capi.calibrate_rng(seed, ids, t, purpose, count)
    for t in range(iterations):
        jump = jump_every > 0 and t % jump_every == jump_every - 1
        u1, u2, u3 = (rng(t, purpose, W) for purpose in (_capi.INFER_U1, _capi.INFER_U2, _capi.INFER_U3))
        if jump:
            normal = rng(t, _capi.INFER_JITTER, W * d).reshape(E, d, W)
        for half in (0, 1):
            mv = slice(H * half, H * half + H)
            other = H * (1 - half)
            xw = x[:, mv]
            take = lambda j: np.take_along_axis(x, j[..., np.newaxis], axis=1)
            with np.errstate(all='ignore'):
                if not jump:
                    j = other + np.minimum((64.0 * u1[:, mv]).astype(np.int64), H - 1)
                    z = ((1.0 + u2[:, mv]) * (1.0 + u2[:, mv])) * 0.5
                    xj = take(j)
                    prop = xj + z[..., np.newaxis] * (xw - xj)
                    log_z = (d - 1.0) * np.log(z)
                else:
                    a = np.minimum((64.0 * u1[:, mv]).astype(np.int64), H - 1)
                    b = (a + 1 + np.minimum((63.0 * u2[:, mv]).astype(np.int64), H - 2)) % H
                    n = normal[:, :, mv].transpose(0, 2, 1)
                    prop = (xw + (take(other + a) - take(other + b))) + (JITTER * (hi - lo)) * n
                    log_z = 0.0
                inside = ((prop > lo) & (prop < hi)).all(axis=-1)
                if inside.any():
                    lp_y, sat_y = calibrate_target(p, np.where(inside[..., np.newaxis], prop, xw))
                    accept = inside & (np.log(u3[:, mv]) < (log_z + lp_y) - lp[:, mv])
                    x[:, mv] = np.where(accept[..., np.newaxis], prop, xw)
                    lp[:, mv] = np.where(accept, lp_y, lp[:, mv])
                    sat[:, mv] = np.where(accept, sat_y, sat[:, mv])
                    accepted[:, mv, 1 if jump else 0] += accept
            evaluations += inside.sum(axis=1)
        if t < burnin:
            continue
        r = t - burnin
        if r == first_half and first_half > 0:
            sums[:, :, 0] = acc
            acc[:] = 0.0
        c = x - shift
        acc[:, :, 0] = acc[:, :, 0] + c
        acc[:, :, 1] = acc[:, :, 1] + c * c
        if rows and r % thin == 0:
            x_rows[:, r // thin], lp_rows[:, r // thin], sat_rows[:, r // thin] = x, lp, sat
    sums[:, :, 1] = acc
    trajectories = None
    if p['want_trajectories']:
        with np.errstate(all='ignore'):
            trajectories = calibrate_target(p, x, trajectories=True)[2]
    return x_rows, lp_rows, sat_rows, sums, accepted, evaluations, invalid, trajectories


def _assemble_calibrate(p, x, lp, saturated, sums, accepted, evaluations, invalid, trajectories):
    """A SimulateResult from the sampler's outputs: the kept rows, pooled summaries, per-draw diagnostics."""
    from .infer import split_rhat
    E, d = p['E'], p['d']
    iterations = p['burnin'] + p['draws_kept']
    n_jump = sum(1 for t in range(iterations) if p['jump_every'] > 0 and t % p['jump_every'] == p['jump_every'] - 1)
    tried = np.array([iterations - n_jump, n_jump], dtype=np.float64) * WALKERS
    with np.errstate(divide='ignore', invalid='ignore'):
        accept = accepted.sum(axis=1) / tried
    if p['draws_kept'] >= 2:
        rhat, mean_e, sd_e = split_rhat(sums, p['draws_kept'], 0.5 * (p['lo'] + p['hi']))
    else:                                                             # one kept iteration: no first half, no R-hat
        mean_e = sums[:, :, :, 0].sum(axis=(1, 2)) / float(WALKERS)
        sd_e = np.sqrt(np.maximum(sums[:, :, :, 1].sum(axis=(1, 2)) / float(WALKERS) - mean_e * mean_e, 0.0))
        rhat, mean_e = np.full((E, d), np.nan), mean_e + 0.5 * (p['lo'] + p['hi'])
    total = sums[:, :, :, 0].sum(axis=(0, 1, 2)) / float(E * WALKERS * p['draws_kept'])
    res = SimulateResult(unknown=list(p['unknown']), draws=E, walkers=WALKERS, accept=accept, rhat=rhat,
                         rhat_max=float(np.nanmax(rhat)) if np.isfinite(rhat).any() else float('nan'),
                         evals=np.asarray(evaluations, dtype=np.int64), invalid=np.asarray(invalid, dtype=bool),
                         mean_per_draw=mean_e, sd_per_draw=sd_e, draw_ids=p['draw_ids'].astype(np.int64),
                         mean=total + 0.5 * (p['lo'] + p['hi']), x=None, lp=None, draw=None, saturated=None, cov=None,
                         quantiles=None, box=np.stack([p['lo'], p['hi']], axis=1), states=list(p['states']), t=p['T'])
    if x is not None:
        rows = x.reshape(-1, d)
        n = rows.shape[0]
        cut = bounds_cut(n)
        srt = np.sort(rows, axis=0)
        res.update(x=rows, lp=lp.reshape(-1), saturated=np.asarray(saturated, dtype=bool).reshape(-1),
                   draw=np.repeat(p['draw_ids'].astype(np.int64), x.shape[1] * WALKERS), mean=rows.mean(axis=0),
                   cov=np.atleast_2d(np.cov(rows, rowvar=False)) if n > 1 else None,
                   quantiles=np.stack([srt[min(cut, n - 1)], srt[max(n - cut, 0)]], axis=1))
    if trajectories is not None:
        flat = trajectories.reshape(E * WALKERS, p['K'], -1)
        n = flat.shape[0]
        cut = bounds_cut(n)
        srt = np.sort(flat, axis=0)
        res.update(trajectories=trajectories, fit_mean=np.mean(flat, axis=0), fit_bounds=np.stack([srt[cut], srt[n - cut]], axis=-1))
    return res


_CALIBRATE_SIGNATURE = """
    models, states, inputs, forcing, y0, t, draws, bounds : as for ``simulate``; the entries of ``y0`` at unknown states are
                  placeholders (any finite number).  Draw e's random numbers are keyed by the row of ``betas`` it selects,
                  so a subset of the draws reproduces the full run's
    unknown     : 1 to 16 names: 'y0:<state>' is that state's initial value, any other name a parameter -- an input column
                  that is neither a state nor a key of ``forcing``, held constant over the run
    observe, data, obs_points, every, obs_sd : the measurements, as for ``assimilate`` (NaN = missing; point 0 may be observed
                  through ``obs_points``)
    prior       : {unknown: (mean, sd)} independent normal priors in true scale; none: flat inside the box
    unknown_bounds : {unknown: (lo, hi)} in true scale, inside the default box: for a parameter the intersection of the
                  training ranges of the columns that read it, for 'y0:<state>' the state's box
    starts      : None -- ``optimize.start_points(128, lo, hi)`` -- or [128, d] in true scale, strictly inside the box
    burnin, draws_kept, thin : iterations dropped, iterations after them, every ``thin``-th of those is kept
    jump_every  : a jump move instead of the stretch move at every ``jump_every``-th iteration; 0: never
    seed        : of the counter-based random numbers; numpy's stream is not touched
    keep        : 'x' the kept rows, 'trajectories' the final ensemble's trajectories, a list of the two, or None (sums,
                  acceptance and R-hat only)

    Returns a ``SimulateResult`` (a dict with attribute access): x [E * kept * 128, d] in true scale (draw-major, then kept
    row, then walker), lp, draw (the row of ``betas`` a sample came from) and saturated (a clamp or the slope rule acted
    along the sample's trajectory) [E * kept * 128]; pooled over the draws mean [d], cov [d, d], quantiles [d, 2] =
    (sorted[cut], sorted[n - cut]) with ``evaluate``'s cut = floor(0.025 n) + 1; per draw accept [E, 2] (stretch, jump
    acceptance rates), rhat [E, d] (split R-hat over the 128 walkers' halves) and rhat_max, evals [E] trajectories
    integrated, invalid [E] (a start had no finite lp), mean_per_draw, sd_per_draw [E, d]; with 'trajectories' trajectories
    [E, 128, n_states, P] of the final ensemble, fit_mean [n_states, P] and fit_bounds [n_states, P, 2] over (draw, walker).
    Without 'x' the row fields are None and mean comes from the sums."""


def calibrate(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, unknown=None, observe=None,
              data=None, obs_points=None, every=None, obs_sd=None, prior=None, unknown_bounds=None, starts=None, burnin=300,
              draws_kept=200, thin=10, jump_every=8, seed=0, keep='x', device=None):
    """Which initial state and which constant inputs produced a measured run?  One ensemble of 128 walkers per posterior
    draw, on the device (module docstring).

    device      : device index (default: the process's device, as for ``fit``), a backend or a ``_capi.DeviceContext``"""
    p = _prepare_calibrate(models, states, inputs, forcing, y0, t, draws, bounds, unknown, observe, data, obs_points, every,
                           obs_sd, prior, unknown_bounds, starts, burnin, draws_kept, thin, jump_every, seed, keep)
    ctx = _device_context(device)
    return _assemble_calibrate(p, *ctx.calibrate(p))


def calibrate_host(models, states, inputs, forcing=None, y0=None, t=None, draws=None, bounds=None, unknown=None, observe=None,
                   data=None, obs_points=None, every=None, obs_sd=None, prior=None, unknown_bounds=None, starts=None,
                   burnin=300, draws_kept=200, thin=10, jump_every=8, seed=0, keep='x'):
    """``calibrate`` in numpy on this host, vectorised over (draws, the 64 walkers of the moving half): the statement the
    kernel is tested against (module docstring), not a fallback.  Same arguments, same result fields."""
    p = _prepare_calibrate(models, states, inputs, forcing, y0, t, draws, bounds, unknown, observe, data, obs_points, every,
                           obs_sd, prior, unknown_bounds, starts, burnin, draws_kept, thin, jump_every, seed, keep)
    return _assemble_calibrate(p, *_run_calibrate_host(p))


calibrate.__doc__ += _CALIBRATE_SIGNATURE
calibrate_host.__doc__ += _CALIBRATE_SIGNATURE
