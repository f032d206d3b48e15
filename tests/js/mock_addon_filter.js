'use strict';
/* tests/js/mock_addon_filter.js — TEST INFRASTRUCTURE: tests/js/mock_addon_patch.js (left as it is; it extends the same mock object) plus the
 * prefiltered entry points of csrc/ht_napi.cc — cropPairsFilteredDevice, cropSourcesFilteredDevice, alignPairsFilteredDevice,
 * alignSourcesFilteredDevice, cropFilterFactors, alignFilterFactors — so that ccv.DeviceBatch's opts.prefilter runs without a GPU.  A
 * filtered call IS, per entry, the mock's own RGBA call of the same name at the fine size Nx P x Ny Q (the factors restated here from the
 * entry's record) followed by the integer block mean; then the RGBA call of the whole list (for the records), and — with a format — the
 * mock's own tensor call on the filtered bytes.  Needs withCrop, withAlign and withPatch.  `withFilter(false)`: an addon without the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_patch.js'));
function factor(num, den, mf) { const need = Math.floor((num + den - 1) / den); return Math.min(mf, Math.max(1, need)); }
function cropFactors(records, i, P, Q, mf) {
  if (records[6 * i] !== 1) return [0, 0];
  return [factor(records[6 * i + 4], P, mf), factor(records[6 * i + 5], Q, mf)];
}
function alignFactors(records, terms, i, P, Q, mf) {
  if (records[4 * i] !== 1) return [0, 0];
  const t = terms.subarray(6 * i, 6 * i + 6);
  return [factor(Math.abs(t[2]) + Math.abs(t[3]), P * 65536, mf), factor(Math.abs(t[4]) + Math.abs(t[5]), Q * 65536, mf)];
}
function checkArgs(w, h, mf) {
  if (!(Number.isInteger(w) && Number.isInteger(h) && Number.isInteger(mf))) throw new TypeError('mock addon: width, height and maxFactor are integers');
  if (w < 1 || w > 1024 || h < 1 || h > 1024 || mf < 1 || mf > 8) throw new RangeError('mock addon: width and height are 1..1024, maxFactor is 1..8');
}
function blockMean(fine, P, Q, nx, ny, dst, at) {
  const n = nx * ny, W = nx * P;
  for (let y = 0; y < Q; y++) for (let x = 0; x < P; x++) for (let ch = 0; ch < 4; ch++) {
    let s = 0;
    for (let b = 0; b < ny; b++) for (let a = 0; a < nx; a++) s += fine[4 * ((ny * y + b) * W + nx * x + a) + ch];
    dst[at + 4 * (y * P + x) + ch] = Math.floor((s + (n >> 1)) / n);
  }
}
/* listAt: 1 (pairs: ctx, pairs, prm, mf, fmt, out, stride, off, wait) or 2 (sources: ctx, streams, entries, prm, mf, fmt, out, stride, off, wait) */
function filteredCall(name, rgbaName, tensorName, resultName, align, listAt) {
  return function () {
    const a = Array.prototype.slice.call(arguments);
    const prm = a[listAt + 1], mf = a[listAt + 2], fmt = a[listAt + 3], out = a[listAt + 4], ostride = a[listAt + 5], ooff = a[listAt + 6] || 0;
    if (!(prm instanceof Int32Array) || prm.length !== 4) throw new TypeError('mock addon: params is an Int32Array of four');
    checkArgs(prm[0], prm[1], mf);
    if (!out || out.kind !== 'dev' || !out.buf) throw new TypeError('mock addon: expected a live device buffer');
    const counts = Object.assign({}, mock.calls);
    const P = prm[0], Q = prm[1], n = listAt === 1 ? a[1].length >> 1 : a[2].length, pb = P * Q * 4;
    const one = function (i) { return listAt === 1 ? [a[0], a[1].subarray(2 * i, 2 * i + 2)] : [a[0], a[1].subarray(i, i + 1), [a[2][i]]]; };
    const filtered = new Uint8Array(n * pb);
    for (let i = 0; i < n; i++) {
      mock[rgbaName].apply(mock, one(i).concat([prm, { kind: 'dev', buf: new Uint8Array(pb) }, 0, 0, false]));
      const r = mock[resultName](a[0], 1);
      const f = align ? alignFactors(r.records, r.terms, 0, P, Q, mf) : cropFactors(r.records, 0, P, Q, mf);
      if (f[0] === 0) continue; /* an empty entry: zeros */
      const fine = { kind: 'dev', buf: new Uint8Array(f[0] * P * f[1] * Q * 4) };
      mock[rgbaName].apply(mock, one(i).concat([Int32Array.from([f[0] * P, f[1] * Q, prm[2], prm[3]]), fine, 0, 0, false]));
      blockMean(fine.buf, P, Q, f[0], f[1], filtered, i * pb);
    }
    const orig = mock[rgbaName], whole = a.slice(0, listAt + 2);
    if (fmt === null || fmt === undefined) {
      if (ostride && (ostride % 4 || ostride < pb)) throw new Error('mock addon: status -1: output stride smaller than a patch or not a multiple of 4');
      const stride = ostride || pb;
      if (ooff + (n - 1) * stride + pb > out.buf.length) throw new RangeError('mock addon: output outside the device buffer');
      orig.apply(mock, whole.concat([{ kind: 'dev', buf: new Uint8Array(n * pb) }, 0, 0, false])); /* the list's records */
      for (let i = 0; i < n; i++) out.buf.set(filtered.subarray(i * pb, (i + 1) * pb), ooff + i * stride);
    } else {
      /* the mock's own tensor call, its RGBA call serving the filtered bytes (and, through the real one, the list's records) */
      mock[rgbaName] = function () { orig.apply(mock, arguments); arguments[listAt + 2].buf.set(filtered); };
      try { mock[tensorName].apply(mock, whole.concat([fmt, out, ostride, ooff, false])); } finally { mock[rgbaName] = orig; }
    }
    mock.calls = counts; /* the facade called this entry point and nothing else */
    mock.calls[name] = (mock.calls[name] || 0) + 1;
  };
}
const filter = {
  cropPairsFilteredDevice: filteredCall('cropPairsFilteredDevice', 'cropPairsDevice', 'cropPairsTensorDevice', 'cropResult', false, 1),
  cropSourcesFilteredDevice: filteredCall('cropSourcesFilteredDevice', 'cropSourcesDevice', 'cropSourcesTensorDevice', 'cropResult', false, 2),
  alignPairsFilteredDevice: filteredCall('alignPairsFilteredDevice', 'alignPairsDevice', 'alignPairsTensorDevice', 'alignResult', true, 1),
  alignSourcesFilteredDevice: filteredCall('alignSourcesFilteredDevice', 'alignSourcesDevice', 'alignSourcesTensorDevice', 'alignResult', true, 2),
  cropFilterFactors: function (records, w, h, mf) {
    if (!(records instanceof Int32Array) || records.length % 6) throw new TypeError('mock addon: records is an Int32Array of 6 n');
    checkArgs(w, h, mf);
    const out = new Int32Array(records.length / 3);
    for (let i = 0; i < records.length / 6; i++) out.set(cropFactors(records, i, w, h, mf), 2 * i);
    return out;
  },
  alignFilterFactors: function (records, terms, w, h, mf) {
    if (!(records instanceof Int32Array) || records.length % 4 || !(terms instanceof Float64Array) || terms.length * 4 !== records.length * 6)
      throw new TypeError('mock addon: records is an Int32Array of 4 n, terms a Float64Array of 6 n');
    checkArgs(w, h, mf);
    const out = new Int32Array(records.length / 2);
    for (let i = 0; i < records.length / 4; i++) out.set(alignFactors(records, terms, i, w, h, mf), 2 * i);
    return out;
  }
};
mock.withFilter = function (on) {
  Object.keys(filter).forEach(function (k) { if (on) mock[k] = filter[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
