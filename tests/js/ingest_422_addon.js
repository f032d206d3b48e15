'use strict';
/* The N-API shim's YUV entry points with the packed 4:2:2 formats, on the CPU (driven by tests/test_ingest_422_addon_cpu.py):
 *     node tests/js/ingest_422_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + draw_list_stub.cc + ingest_422_stub.cc>
 * Successful calls (what reaches the C ABI is in the stubs' logs) and malformed ones (the message each one throws is printed): a 4:2:2 frame
 * is 4 * ceil(w / 2) * h bytes — a buffer that exactly fits passes, one byte short throws —, its one plane is y / p0, and an offset that is
 * no multiple of 4 is refused with a message.  Prints one JSON line. */
const A = require(process.argv[2]);
const out = { consts: [A.YUV_YUYV, A.YUV_UYVY, A.YUV_NV12, A.YUV_I420, A.DRAW_RGBA], thrown: [] };
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const fb = 40 * 30 * 4, W = 23, H = 7, F = 4 * 12 * 7;                                     /* 23 x 7: 12 macropixels per row, 336 bytes */
const fill = function (n) { const a = new Uint8Array(n); for (let i = 0; i < n; i++) a[i] = (i * 7 + 3) & 255; return a; };
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }

/* drawFramesYuv(ctx, planes, n, w, h, format, matrix, rect): the host form */
A.drawFramesYuv(c, fill(2 * F), 2, W, H, A.YUV_YUYV, 1, null);                              /* exactly fits */
A.drawFramesYuv(c, fill(F + 9), 1, W, H, A.YUV_UYVY, 3, Int32Array.from([1, 1, 21, 5]));   /* longer than needed, a rect */
A.drawFramesYuv(c, fill(1 * 1 + 2), 1, 1, 1, A.YUV_I420, 0, null);                          /* 4:2:0 is sized as before: 3 bytes */
bad('host form one byte short', function () { A.drawFramesYuv(c, fill(2 * F - 1), 2, W, H, A.YUV_YUYV, 1, null); });
bad('host form: a 4:2:0-sized buffer is too short for 4:2:2', function () { A.drawFramesYuv(c, fill(W * H + 2 * 12 * 4), 1, W, H, A.YUV_UYVY, 0, null); });

/* drawFramesYuvDevice(ctx, srcDev, srcOffset, n, w, h, format, matrix, stride, rect, dstDev, dstOffset, dstStride, wait) */
const src = A.deviceAlloc(c, 8 + 3 * F), dst = A.deviceAlloc(c, 3 * fb);
A.drawFramesYuvDevice(c, src, 8, 3, W, H, A.YUV_YUYV, 2, 0, null, dst, 0, 0, false);        /* three packed frames, the buffer's last bytes */
A.drawFramesYuvDevice(c, src, 4, 2, W, H, A.YUV_UYVY, 0, F + 8, Int32Array.from([0, 0, 2, 2]), null, 0, 0, false);  /* a stride with a gap; the bind form */
A.drawFramesYuvDevice(c, src, 1, 1, W, H, A.YUV_NV12, 0, 0, null, dst, 0, 0, false);        /* 4:2:0 needs no aligned offset and has its chroma plane */
bad('device form one byte beyond', function () { A.drawFramesYuvDevice(c, src, 12, 3, W, H, A.YUV_YUYV, 2, 0, null, dst, 0, 0, false); });
bad('device form misaligned offset', function () { A.drawFramesYuvDevice(c, src, 6, 1, W, H, A.YUV_YUYV, 2, 0, null, dst, 0, 0, false); });
bad('device form: stride with a gap beyond', function () { A.drawFramesYuvDevice(c, src, 8, 3, W, H, A.YUV_UYVY, 0, F + 4, null, dst, 0, 0, false); });

/* drawListDevice: a packed entry is p0 alone */
const yuyv = { dev: src, offset: 8, width: W, height: H, format: A.YUV_YUYV, matrix: 1, rect: null };
const uyvy = { dev: src, offset: 8 + 2 * F, width: W, height: H, format: A.YUV_UYVY, matrix: 2, rect: Int32Array.from([3, 1, 20, 6]) };  /* the buffer's last frame */
const nv12 = { dev: src, offset: 9, width: 5, height: 3, format: A.YUV_NV12, matrix: 0 };
A.drawListDevice(c, [yuyv, nv12, uyvy, yuyv], null, 0);  /* the bind form (four entries: the recording stub refuses exactly three) */
bad('list entry one byte beyond', function () { A.drawListDevice(c, [yuyv, Object.assign({}, uyvy, { offset: 8 + 2 * F + 4 })], dst, 0); });
bad('list entry misaligned offset', function () { A.drawListDevice(c, [yuyv, Object.assign({}, uyvy, { offset: 8 + F + 2 })], dst, 0); });
A.drawListDevice(c, [uyvy, yuyv], dst, 0);
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
