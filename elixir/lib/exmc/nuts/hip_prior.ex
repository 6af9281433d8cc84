defmodule Exmc.NUTS.HipPrior do
  @moduledoc """
  `Exmc.Predictive.prior_samples/3` of a built model kind on the device (DESIGN.md "Prior predictive"):
  every chain's draws are made by one generator in one kernel launch
  (`Exmc.NUTS.HipPriorNative.prior_samples/6`), bit-identical to the statement of `predictive.ex` and the
  `sample/2` callbacks it calls.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5` (it carries `{kind, data}`); `n` is the
  number of draws; opts `:num_chains` (1), `:seed` (0), `:chain_lo` (0: a caller that shards its chains
  offsets the seeds with it), `:var_names` (the kind's free variables in kernel order; the default names
  them as the kinds' own models do, radon's county intercepts as `"alpha_raw_<k>"` in the kind's data
  order) and `:replicates` (true). Returns per chain what the reference returns: a list of
  `%{var_name => Nx.t({n})}`, one map per chain, chain c drawn with `seed + 7919 * (chain_lo + c)`; with
  one chain the map itself. With `replicates: true` the map also holds the prior predictive replicates of
  every datum under the keys of `Exmc.NUTS.HipPredictive` (`opts[:names]` replaces them).

  Deviations from the reference: within a draw the free variables are walked in the reference's Kahn
  order and the datums follow in the kind's data order; the tangent of HalfCauchy is that of the exact
  (pi/2) u; a uniform of exactly 0.0 gives `:infinity` in effect from Exponential and 0.0 from
  HalfCauchy; for sv_ncp the values of `s_2 .. s_100` are the reconstructed walk; generated models raise
  `{:exmc_hip_error, 4, _}`.
  """

  alias Exmc.NUTS.{HipPredictive, HipPriorNative}

  def prior_samples(%{model: model}, n \\ 100, opts \\ []) do
    c = Keyword.get(opts, :num_chains, 1)
    rep = if Keyword.get(opts, :replicates, true), do: 1, else: 0
    {x, _q, yrep} = HipPriorNative.prior_samples(model, c, n, Keyword.get(opts, :seed, 0), Keyword.get(opts, :chain_lo, 0), rep)
    d = div(byte_size(x), 8 * c * n)
    vars = Keyword.get(opts, :var_names) || var_names(elem(model, 0), d)
    nd = div(byte_size(yrep), 8 * c * n)
    datums = if rep == 1, do: Keyword.get(opts, :names) || HipPredictive.datum_names(elem(model, 0), nd), else: []

    maps =
      for ch <- 0..(c - 1) do
        xs = columns(x, ch, n, d, vars)
        ys = if rep == 1, do: columns(yrep, ch, n, nd, datums), else: %{}
        Map.merge(xs, ys)
      end

    if c == 1, do: hd(maps), else: maps
  end

  # [draw][column] of the chain -> one {n} tensor per column
  defp columns(bin, ch, n, w, names) do
    t = binary_part(bin, ch * n * w * 8, n * w * 8) |> Nx.from_binary(:f64) |> Nx.reshape({n, w})
    names |> Enum.with_index() |> Map.new(fn {name, i} -> {name, t[[.., i]]} end)
  end

  # the kinds of include/exmc_hip.h in kernel order: 1 simple, 2 eight_schools, 3 sv, 4 logistic, 5 radon,
  # 7 sv_ncp
  @doc false
  def var_names(1, _d), do: ["mu", "sigma"]
  def var_names(2, _d), do: ["mu", "tau"] ++ for(j <- 0..7, do: "theta_trans_#{j}")
  def var_names(kind, _d) when kind in [3, 7], do: for(t <- 1..100, do: "s_#{t}") ++ ["sigma", "nu"]
  def var_names(4, d), do: ["alpha"] ++ for(j <- 1..(d - 1), do: "beta_#{j}")

  def var_names(5, d),
    do: for(k <- 0..(d - 6), do: "alpha_raw_#{k}") ++ ["mu_alpha", "gamma_u", "sigma_alpha", "sigma_y", "beta"]
end
