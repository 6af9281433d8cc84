defmodule Exmc.NUTS.HipPsisNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s PSIS-LOO (`include/exmc_hip_psis.h`, DESIGN.md "PSIS-LOO"): the
  Pareto-smoothed importance-sampling LOO of a built model kind with the Pareto k of every datum,
  computed on the device. The C side is `c_src/exmc_hip_psis_nif.c`, a module beside
  `Exmc.NUTS.HipCompareNative` (whose table it leaves as it is); conventions are HipNative's.

  Load: `priv/exmc_hip_psis_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_psis_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; draws: `[chain][draw][dim]` f64
  binary in kernel order, as HipNative's sampling functions return it -> `[3][N]` f64 binary, rows
  elpd_loo, p_loo and the Pareto k of every datum (+inf: tail too short to fit; NaN in all three rows:
  a non-finite term), datums in the kind's data order
  """
  def psis_stats(_model, _draws, _n_chains, _n_draws), do: :erlang.nif_error(:nif_not_loaded)
end
