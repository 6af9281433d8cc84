defmodule Exmc.NUTS.HipPpcNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s posterior predictive checks (`include/exmc_hip_ppc.h`, DESIGN.md
  "Posterior predictive checks"): the replicates of `Exmc.NUTS.HipPredictiveNative` reduced on the device
  to per-datum summaries and Bayesian p-values, the replicate matrix never formed. The C side is
  `c_src/exmc_hip_ppc_nif.c`, a module beside `Exmc.NUTS.HipPredictiveNative`; conventions are
  HipNative's. `Exmc.NUTS.HipPpc.ppc/3` is the caller.

  Load: `priv/exmc_hip_ppc_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_ppc_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; draws: `[chain][draw][dim]` f64
  binary in kernel order; chain c draws with seed + 7919 (chain_lo + c) ->
  `{datum_bin [datum][4] (mean, var, p_lt, p_eq), t_obs_bin [4], p_value_bin [4]}`, f64 binaries, the
  statistics mean, var, min, max, the datums in the kind's data order
  """
  def ppc(_model, _draws, _n_chains, _n_draws, _seed, _chain_lo),
    do: :erlang.nif_error(:nif_not_loaded)
end
