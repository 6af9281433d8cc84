defmodule Exmc.NUTS.HipSampler do
  @moduledoc """
  The HIP branch of `Exmc.NUTS.Sampler` / `Exmc.Compiler.compile_for_sampling/2`: what the two
  patches under `elixir/patches/` call when `Application.get_env(:exmc, :hip, false)`.

  A compiled model is `%{ref: handle, pm: %Exmc.PointMap{}, ncp_info: map, perm: [integer]}`:
  `ref` is a `HipNative` model handle (one of the built kinds, or a plug-in generated from the IR),
  `perm` the kernel dimension of every flat (PointMap) entry. Traces come back from the device as
  `[chain][draw][dim]` f64 binaries in KERNEL order; `flat_draws/4` reorders a chain's rows into the
  flat order `build_trace/3` (`sampler.ex:1281-1298`) slices, so the constrained traces, the
  NCP reconstruction and the stats maps are produced by the reference's own unchanged code.
  """

  alias Exmc.NUTS.{HipCompareNative, HipExport, HipNative}

  @default_opts [num_warmup: 1000, num_samples: 1000, max_tree_depth: 10, target_accept: 0.8, seed: 0]

  @doc "The probe `Tree.nif_available?/0` (tree.ex:52-54) has, for this library."
  def available? do
    Application.get_env(:exmc, :hip, false) and Code.ensure_loaded?(HipNative) and
      function_exported?(HipNative, :model_create, 2) and nif_loaded?()
  end

  defp nif_loaded? do
    try do
      HipNative.model_create(-1, <<>>)
      true
    rescue
      ErlangError -> false
      ArgumentError -> true
    end
  end

  @doc """
  compile_for_sampling/2, HIP branch (compiler.ex:46-58): export the rewritten IR, generate and build
  the plug-in (cached by the digest of the generated text), load it through the NIF.
  `dir` is a scratch directory for model.json.in / model.json / the library.
  """
  def compile(%Exmc.IR{} = ir, pm, ncp_info, dir, opts \\ []) do
    json = HipExport.to_json(Exmc.Rewrite.apply(ir, ncp: false), Keyword.get(opts, :ncp, true))
    File.mkdir_p!(dir)
    File.write!(Path.join(dir, "model.json.in"), json)
    {_, 0} = System.cmd("python3", ["-m", "exmc_amd.codegen", Path.join(dir, "model.json.in"), dir])
    meta = dir |> Path.join("model.json") |> File.read!() |> Jason.decode!()
    data = for x <- meta["data"], into: <<>>, do: <<x::float-64-native>>
    {:ok, ref} = HipNative.model_create_plugin(Path.join(dir, meta["library"]), data)
    # the generator lays the free variables out in PointMap order already: identity permutation
    %{ref: ref, pm: pm, ncp_info: ncp_info, perm: Enum.to_list(0..(pm.size - 1)), meta: meta}
  end

  @doc "One of the built kinds (include/exmc_hip.h model kinds); `perm` as model_set_flat_order/2 takes it."
  def compile_kind(kind, data_bin, pm, ncp_info, perm) do
    {:ok, ref} = HipNative.model_create(kind, data_bin)
    :ok = HipNative.model_set_flat_order(ref, perm)
    # kind and data ride along for model comparison (waic/3, loo/3: HipCompareNative.ic_stats/4; psis_loo/3: HipPsisNative.psis_stats/4)
    %{ref: ref, pm: pm, ncp_info: ncp_info, perm: perm, model: {kind, data_bin}}
  end

  @doc """
  sample_from_compiled/3 (sampler.ex:126-257), one chain: adaptation and draws as ONE NIF call. opts[:dense_mass]
  (sampler.ex:156) and opts[:warm_start] (sampler.ex:167-197; the `stats` of a previous run: `inv_mass_diag` in
  flat order as every stats map reports it, `step_size`) pick the call. Returns `{tuning, flat draws, trace_map}`;
  `tuning.inv_mass_diag` is the flat-order tensor for the stats map, `tuning.warmup_divergences` the warmup's share
  of `stats.divergences` (sampler.ex:245 counts both phases); a dense tuning also carries `:cov` / `:chol_cov`.
  """
  def sample(%{ref: ref} = compiled, opts) do
    opts = Keyword.merge(@default_opts, opts)
    init_q = init_q(compiled, Keyword.get(opts, :init_q))
    {nw, ns, depth, accept, seed} =
      {opts[:num_warmup], opts[:num_samples], opts[:max_tree_depth], opts[:target_accept], opts[:seed]}

    {trace, tuning, _divergences} =
      cond do
        Keyword.get(opts, :dense_mass, false) ->
          HipNative.sample_dense(ref, init_q, nw, ns, depth, accept, seed, 0)

        ws = Keyword.get(opts, :warm_start) ->
          prev_im = kernel_inv_mass(compiled, ws.inv_mass_diag)
          HipNative.sample_warm(ref, init_q, nw, ns, depth, accept, seed, ws.step_size * 1.0, prev_im)

        true ->
          HipNative.sample(ref, init_q, nw, ns, depth, accept, seed)
      end

    tuning = Map.put(tuning, :inv_mass_diag, flat_inv_mass(compiled, tuning.inv_mass))
    [draws] = chains(compiled, trace, 1, opts[:num_samples])
    {tuning, draws, trace}
  end

  @doc """
  sample_from_compiled_tuned/4 (sampler.ex:259-335; `sample_compiled_tuned/4`, and what
  `Distributed.run_chain_remote` calls): no warmup, the draws of one chain under the tuning map
  `%{epsilon, inv_mass, chol_cov}` of the reference -- `inv_mass` a flat-order `{d}` tensor, or the `{d, d}`
  covariance together with its Cholesky factor `chol_cov` for a dense mass (sampler.ex:274, 292).
  Returns `{flat draws, trace_map}`.
  """
  def sample_tuned(%{ref: ref, pm: pm} = compiled, tuning, opts) do
    opts = Keyword.merge(@default_opts, opts)
    init_q = init_q(compiled, Keyword.get(opts, :init_q))
    d = pm.size

    diag =
      case Map.get(tuning, :chol_cov) do
        nil ->
          :ok = HipNative.clear_dense_mass(ref)
          tuning.inv_mass

        chol ->
          f64 = fn t -> t |> Nx.as_type(:f64) |> Nx.reshape({d * d}) |> Nx.to_binary() end
          :ok = HipNative.set_dense_mass(ref, f64.(tuning.inv_mass), f64.(chol))
          Nx.take_diagonal(tuning.inv_mass)
      end

    {trace, _leapfrogs, _divergences} =
      HipNative.sample_chains(ref, tuning.epsilon * 1.0, kernel_inv_mass(compiled, diag), init_q, 1, 0, 1,
        opts[:num_samples], opts[:max_tree_depth], opts[:seed])

    [draws] = chains(compiled, trace, 1, opts[:num_samples])
    {draws, trace}
  end

  @doc """
  sample_chains_vectorized_compiled/3 (sampler.ex:1020-1136): the shared warmup on chain 0, then
  every chain with its tuning, as two NIF calls. Returns `{tuning, [flat draws per chain], trace_map}`;
  the caller builds traces and stats with its own build_trace/3.
  """
  def sample_chains_vectorized(%{ref: ref} = compiled, num_chains, opts) do
    opts = Keyword.merge(@default_opts, opts)
    init_q = init_q(compiled, Keyword.get(opts, :init_q))

    tuning =
      HipNative.warmup(ref, init_q, opts[:num_warmup], opts[:max_tree_depth], opts[:target_accept], opts[:seed])

    {trace, _leapfrogs, _divergences} =
      HipNative.sample_chains(ref, tuning.epsilon, tuning.inv_mass, init_q, num_chains, 0, num_chains,
        opts[:num_samples], opts[:max_tree_depth], opts[:seed])

    # tuning.inv_mass stays in KERNEL order (it goes back into HipNative.sample_chains above);
    # stats.inv_mass_diag is reported in the flat order of the trace, as the reference's is
    tuning = Map.put(tuning, :inv_mass_diag, flat_inv_mass(compiled, tuning.inv_mass))
    {tuning, chains(compiled, trace, num_chains, opts[:num_samples]), trace}
  end

  @doc """
  sample_chains_parallel (sampler.ex:1139-1176), `vectorized: false`: every chain its own adaptation,
  one launch. Returns `{[tuning per chain], [flat draws per chain], trace_map}`.
  """
  def sample_chains_independent(%{ref: ref, pm: pm} = compiled, num_chains, opts) do
    opts = Keyword.merge(@default_opts, opts)
    init_q = init_q(compiled, Keyword.get(opts, :init_q))

    {trace, tuning_bin, _leapfrogs, _divergences} =
      HipNative.sample_independent(ref, init_q, num_chains, 0, num_chains, opts[:num_warmup], opts[:num_samples],
        opts[:max_tree_depth], opts[:target_accept], opts[:seed])

    d = pm.size
    row = (3 + d) * 8

    tunings =
      for c <- 0..(num_chains - 1) do
        <<eps::float-64-native, wdiv::float-64-native, _wlf::float-64-native, im::binary-size(d * 8)>> =
          binary_part(tuning_bin, c * row, row)

        %{epsilon: eps, warmup_divergences: trunc(wdiv), inv_mass: im, inv_mass_diag: flat_inv_mass(compiled, im)}
      end

    {tunings, chains(compiled, trace, num_chains, opts[:num_samples]), trace}
  end

  @doc "sample_stream/4 (sampler.ex:1186-1277): warmup, then ONE launch whose draws arrive as messages."
  def sample_stream(%{ref: ref} = compiled, receiver_pid, opts) do
    opts = Keyword.merge(@default_opts, opts)
    init_q = init_q(compiled, Keyword.get(opts, :init_q))
    _tuning = HipNative.stream_begin(ref, init_q, opts[:num_warmup], opts[:max_tree_depth], opts[:target_accept], opts[:seed])
    HipNative.stream_run(ref, opts[:num_samples], receiver_pid)
  end

  # ---- model comparison (Exmc.ModelComparison, model_comparison.ex) ----

  @doc """
  `ModelComparison.waic/1` of a built kind over the datums of its data (one y_i, one return r_t;
  DESIGN.md "Model comparison"): `draws` is the `[chain][draw][dim]` kernel-order binary the sampling
  functions return (`trace.draws` of `sample_chains_vectorized/3`), opts `:num_chains` and
  `:num_draws`. The per-datum statistics come from the device (`HipCompareNative.ic_stats/4`), the
  totals from the reference's formulas -> `%{waic:, elpd_waic:, p_waic:, se:, n_obs:}`. A compiled
  model of `compile_kind/5` only: a generated model has no per-datum terms
  (`{:exmc_hip_error, 4, _}`).
  """
  def waic(%{model: model}, draws, opts) do
    {lppd, p_waic, _elpd_loo, _p_loo} = ic_rows(model, draws, opts)
    n = length(lppd)
    lp = Enum.sum(lppd)
    pw = Enum.sum(p_waic)
    elpd_waic = lp - pw
    elpd_pointwise = Enum.zip_with(lppd, p_waic, fn l, p -> l - p end)
    se = if n > 1, do: :math.sqrt(n * variance(elpd_pointwise)), else: 0.0
    %{waic: -2 * elpd_waic, elpd_waic: elpd_waic, p_waic: pw, se: se, n_obs: n}
  end

  @doc "`ModelComparison.loo/1` (plain importance-sampling LOO) the same way -> `%{loo:, elpd_loo:, p_loo:, se:, n_obs:}`"
  def loo(%{model: model}, draws, opts) do
    {_lppd, _p_waic, elpd_loo, p_loo} = ic_rows(model, draws, opts)
    n = length(elpd_loo)
    elpd = Enum.sum(elpd_loo)
    se = if n > 1, do: :math.sqrt(n * variance(elpd_loo)), else: 0.0
    %{loo: -2 * elpd, elpd_loo: elpd, p_loo: Enum.sum(p_loo), se: se, n_obs: n}
  end

  @doc """
  Pareto-smoothed importance-sampling LOO (DESIGN.md "PSIS-LOO") the same way ->
  `%{loo:, elpd_loo:, p_loo:, se:, n_obs:, pareto_k:, k_threshold:, n_high_k:}`: `pareto_k` is the list of
  the datums' Pareto k (`:infinity` where the tail was too short to fit, `:nan` for a datum with a non-finite term), `k_threshold`
  min(1 - 1/log10(n), 0.7) for n = num_chains * num_draws, `n_high_k` the number of datums not at or below it (`:infinity` and `:nan` count).
  """
  def psis_loo(%{model: model}, draws, opts) do
    num_chains = Keyword.fetch!(opts, :num_chains)
    num_draws = Keyword.fetch!(opts, :num_draws)
    out = Exmc.NUTS.HipPsisNative.psis_stats(model, draws, num_chains, num_draws)
    # +inf and NaN are not Erlang floats: decode them as atoms
    vals =
      for <<bits::64-native <- out>> do
        case <<bits::64-native>> do
          <<x::float-64-native>> -> x
          _ -> if Bitwise.band(bits, 0x000FFFFFFFFFFFFF) == 0, do: :infinity, else: :nan
        end
      end

    n = div(length(vals), 3)
    [elpd_loo, p_loo, k] = Enum.chunk_every(vals, n)
    thr = min(1.0 - 1.0 / :math.log10(num_chains * num_draws), 0.7)
    finite = Enum.all?(elpd_loo ++ p_loo, &is_float/1)
    elpd = if finite, do: Enum.sum(elpd_loo), else: :nan
    se = if finite and n > 1, do: :math.sqrt(n * variance(elpd_loo)), else: if(finite, do: 0.0, else: :nan)

    %{
      loo: if(finite, do: -2 * elpd, else: :nan),
      elpd_loo: elpd,
      p_loo: if(finite, do: Enum.sum(p_loo), else: :nan),
      se: se,
      n_obs: n,
      pareto_k: k,
      k_threshold: thr,
      n_high_k: Enum.count(k, fn v -> not (is_float(v) and v <= thr) end)
    }
  end

  defp ic_rows(model, draws, opts) do
    stats = HipCompareNative.ic_stats(model, draws, Keyword.fetch!(opts, :num_chains), Keyword.fetch!(opts, :num_draws))
    vals = for <<x::float-64-native <- stats>>, do: x
    n = div(length(vals), 4)
    [a, b, c, d] = Enum.chunk_every(vals, n)
    {a, b, c, d}
  end

  # model_comparison.ex:260-269
  defp variance(values) do
    n = length(values)

    if n < 2 do
      0.0
    else
      mean = Enum.sum(values) / n
      Enum.sum(Enum.map(values, fn x -> (x - mean) * (x - mean) end)) / (n - 1)
    end
  end

  # ---- layout helpers ----

  # [chain][draw][dim] kernel-order binary -> per chain a list of flat-order f64 row tensors
  defp chains(%{pm: pm, perm: perm}, %{draws: draws}, num_chains, num_samples) do
    d = pm.size
    chain_bytes = num_samples * d * 8

    for c <- 0..(num_chains - 1) do
      flat_draws(binary_part(draws, c * chain_bytes, chain_bytes), num_samples, d, perm)
    end
  end

  @doc """
  A kernel-order inverse mass diagonal (f64 binary, as the NIF returns it) as the `{d}` tensor
  `stats.inv_mass_diag` carries: flat (PointMap) order, the order of the trace. For the built kinds
  `perm` is not the identity (e.g. radon's counties by size, sv's string sort).
  """
  def flat_inv_mass(%{perm: perm}, inv_mass_bin) do
    Nx.from_binary(inv_mass_bin, :f64) |> Nx.take(Nx.tensor(perm, type: :s64))
  end

  @doc """
  The inverse of `flat_inv_mass/2`: a flat-order `{d}` tensor (what `stats.inv_mass_diag` holds, e.g. inside
  opts[:warm_start]) as the kernel-order f64 binary the NIFs take. Kernel dimension perm[r] takes flat entry r.
  """
  def kernel_inv_mass(%{perm: perm}, %Nx.Tensor{} = flat) do
    vals = flat |> Nx.as_type(:f64) |> Nx.to_flat_list()

    perm
    |> Enum.zip(vals)
    |> Enum.sort()
    |> Enum.reduce(<<>>, fn {_k, x}, acc -> <<acc::binary, x::float-64-native>> end)
  end

  @doc false
  def flat_draws(chain_bin, num_samples, d, perm) do
    t = Nx.from_binary(chain_bin, :f64) |> Nx.reshape({num_samples, d})
    idx = Nx.tensor(perm, type: :s64)
    # flat entry r = kernel dimension perm[r]
    Nx.take(t, idx, axis: 1)
  end

  # opts[:init_q]: the flat unconstrained start the sampler's own init_position/5 computed from
  # opts[:init_values] (sampler.ex:351-356: NCP inversion, to_unconstrained, pack), or nil for the
  # random start (0.1 * normal_s per flat entry, drawn on the device from the chain's seed)
  defp init_q(_compiled, nil), do: nil

  defp init_q(%{perm: perm}, %Nx.Tensor{} = flat_q) do
    flat = flat_q |> Nx.as_type(:f64) |> Nx.to_flat_list()
    # kernel dimension perm[r] takes flat entry r
    kernel =
      perm
      |> Enum.with_index()
      |> Enum.sort()
      |> Enum.map(fn {_k, r} -> Enum.at(flat, r) end)

    for x <- kernel, into: <<>>, do: <<x::float-64-native>>
  end
end
