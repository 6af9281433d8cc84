defmodule Exmc.NUTS.HipLooPit do
  @moduledoc """
  PSIS-LOO-PIT of a built model kind on the device (DESIGN.md "LOO-PIT"): the probability integral
  transform of every observation under its leave-one-out predictive distribution. The replicates are those
  `Exmc.NUTS.HipPredictive.posterior_predictive/3` would return at the same seed, each weighted with the
  Pareto-smoothed importance weight of its sample as PSIS-LOO forms it
  (`Exmc.NUTS.HipLooPitNative.loo_pit/6`); neither the replicate nor the pointwise matrix is kept.

  The model is a map of `Exmc.NUTS.HipSampler.compile_kind/5`; `trace` is the `[chain][draw][dim]`
  kernel-order binary the sampling functions return, opts `:num_chains` and `:num_draws`, `:seed` (0)
  and `:chain_lo` (0: it only seeds the generators; the weights pool all chains of the call, so a shard of
  the chains is another estimator). Returns

      %{datum_key => %{p_lt: float, p_eq: float, pit: float, k: float}}

  with the keys of `Exmc.NUTS.HipPredictive` (`opts[:names]`, a list of N keys, replaces them): the
  weighted share of replicates below and equal to the observation, `pit = p_lt + 0.5 * p_eq`, and the
  datum's Pareto k. A PIT whose k is above `min(1 - 1 / log10(n), 0.7)` is not to be trusted; k is
  `:infinity` where the tail was too short to smooth, and a datum with a non-finite term has `:nan` in all
  four. Generated models raise `{:exmc_hip_error, 4, _}`.
  """

  alias Exmc.NUTS.{HipLooPitNative, HipPredictive}

  @rows [:p_lt, :p_eq, :pit, :k]

  def loo_pit(%{model: model}, trace, opts \\ []) do
    c = Keyword.fetch!(opts, :num_chains)
    s = Keyword.fetch!(opts, :num_draws)
    out = HipLooPitNative.loo_pit(model, trace, c, s, Keyword.get(opts, :seed, 0), Keyword.get(opts, :chain_lo, 0))
    n = div(byte_size(out), 32)
    names = Keyword.get(opts, :names) || HipPredictive.datum_names(elem(model, 0), n)
    cols = for r <- 0..3, do: binary_part(out, r * n * 8, n * 8) |> floats()

    [names | cols]
    |> Enum.zip()
    |> Map.new(fn {name, p_lt, p_eq, pit, k} -> {name, Map.new(Enum.zip(@rows, [p_lt, p_eq, pit, k]))} end)
  end

  # f64 binary -> floats, the non-finite ones as the atoms Nx uses (:nan, :infinity, :neg_infinity)
  defp floats(bin), do: bin |> Nx.from_binary(:f64) |> Nx.to_flat_list()
end
